"""Cases and references for the fp64 device building blocks (tests/dev_blocks.py, tests/csrc/dev_blocks.hip).

Every continuous block is sampled by ZONE: at least 64 inputs on one side of one branch of the block's text (frames, which are
expensive, come in smaller zones: the listed row counts of one view class).  A zone carries its inputs, the branch variables that
put it on its side (``sides``: checked on the CPU to lie at least 1 % from the switch, see ``check_sides``), and ``measure``, which
turns a block's outputs (the device's, or a host statement's) into the zone's gap against the reference, already divided by the
output's natural size.  The gate is ``gate(g_host)``: see DESIGN.md, "The device building blocks one by one".

References.  Values come from restatements of the documented models in 50-digit mpmath (``mp_rotation``, ``mp_pinhole``,
``mp_fisheye``), which tests/test_dev_blocks_host.py pins to camera_exact.rotation / distort and fisheye_exact.distort (the 64-bit
mantissa statements) and to mpmath.expm.  Derivatives are central differences of those restatements, camera_exact.jacobian_fd's
recipe, but taken in mpmath with a step of 1e-20, so that their own error (1e-30) is far below fp64: with jacobian_fd's step of
1e-6 in long double the reference's error (1e-12) would hide every block's rounding.  Frames' sums (``evaluate``) use
camera_exact.residuals / jacobian_fd and fisheye_exact.project / jacobian_fd as they are.  Spectral references come from
mpmath.eigsy and from the defining properties.  Nothing is imported from deepcharuco_amd/pnp.py or fisheye.py; the thresholds
named here (1e-300, 1e-5, 1e-8, 1e-4) are the ones the device headers spell out, restated to place the zones, and the CPU test
reads them back from the header text."""
import functools
import math
from collections import namedtuple

import mpmath
import numpy as np

import camera_exact as cx
import fisheye_exact as fe

EPS = float(np.finfo(np.float64).eps)
DPS = 50
N = 64                                     # inputs per zone
LD = cx.LD

Zone = namedtuple("Zone", "name x measure sides expect")
Zone.__new__.__defaults__ = ((), None)


def gate(g_host):
    """The device's bound for a zone whose host statement measured ``g_host`` (both already divided by the output's size)."""
    return 8.0 * max(g_host, 4.0 * EPS)


def check_sides(zone):
    """Every branch variable of the zone lies on its side of its switch, at least 1 % away."""
    for label, values, switch, side in zone.sides:
        v = np.asarray(values, np.float64)
        assert v.size, (zone.name, label)
        ok = v < 0.99 * switch if side == "<" else v > 1.01 * switch
        assert ok.all(), (zone.name, label, side, switch, v[~ok][:4])


def _gap(out, ref, groups):
    """max over the groups (columns, scale) of max |out - ref| / scale; NaN in the output counts as infinite."""
    g = 0.0
    for cols, scale in groups:
        d = np.abs(np.asarray(out)[:, cols].astype(LD) - ref[:, cols])
        if np.isnan(d.astype(np.float64)).any():
            return math.inf
        g = max(g, float(d.max()) / scale)
    return g


def _by_ref(ref, groups=None):
    """measure() for a plain reference table: groups of columns, each scaled by the largest reference entry of the group in the
    zone (or by the scale given)."""
    ref = np.asarray(ref)
    if groups is None:
        groups = [(slice(None), None)]
    gs = []
    for cols, scale in groups:
        if scale is None:
            scale = float(np.abs(ref[:, cols].astype(np.float64)).max())
        gs.append((cols, scale if scale > 0 else 1.0))
    return lambda out, iout=None: _gap(out, ref, gs)


def _rng(*key):
    return np.random.default_rng([2024, *key])


def _dirs(rng, n=N):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------------ mpmath restatements

def mpf(v):
    return mpmath.mpf(float(v))


def mp_rotation(r):
    """exp([r]x) as a list of rows, closed form without cancellation (2 sin^2(th/2) for 1 - cos th); r mpf."""
    S = [[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]
    th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    eye = [[mpmath.mpf(i == j) for j in range(3)] for i in range(3)]
    if th2 == 0:
        return [[eye[i][j] + S[i][j] for j in range(3)] for i in range(3)]
    th = mpmath.sqrt(th2)
    a, h = mpmath.sin(th) / th, mpmath.sin(th / 2)
    b = 2 * h * h / th2
    S2 = [[sum(S[i][k] * S[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    return [[eye[i][j] + a * S[i][j] + b * S2[i][j] for j in range(3)] for i in range(3)]


def mp_pinhole(x, y, k):
    """Normalised -> distorted normalised, the documented rational + tangential model; k = k1 k2 p1 p2 k3 k4 k5 k6 (mpf)."""
    r2 = x * x + y * y
    g = (1 + k[0] * r2 + k[1] * r2 ** 2 + k[4] * r2 ** 3) / (1 + k[5] * r2 + k[6] * r2 ** 2 + k[7] * r2 ** 3)
    return [x * g + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x), y * g + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y]


def mp_fisheye(a, b, k):
    """Normalised -> the fisheye model's (x', y'); r = 0 takes the limit 0."""
    r = mpmath.sqrt(a * a + b * b)
    if r == 0:
        return [mpmath.mpf(0), mpmath.mpf(0)]
    th = mpmath.atan(r)
    thd = th * (1 + k[0] * th ** 2 + k[1] * th ** 4 + k[2] * th ** 6 + k[3] * th ** 8)
    return [thd / r * a, thd / r * b]


def mp_fd(f, x, h=None):
    """Central differences of f (list -> list) at x -> J[i][j] = df_i / dx_j."""
    h = mpmath.mpf(10) ** -20 if h is None else h
    cols = []
    for j in range(len(x)):
        xp, xm = list(x), list(x)
        xp[j] = x[j] + h
        xm[j] = x[j] - h
        fp, fm = f(xp), f(xm)
        cols.append([(p - m) / (2 * h) for p, m in zip(fp, fm)])
    return [[cols[j][i] for j in range(len(x))] for i in range(len(cols[0]))]


def _flat(rows):
    return [float(v) for row in rows for v in row]


# ------------------------------------------------------------------------------------------------ rotations

TH_IDENTITY = 1e-300          # rodrigues: below it the identity
S_SMALL = 1e-5                # rvec_of: below it the zero / half-turn arms
TH2_SERIES = 1e-8             # right_jacobian: below it the series


def _rvecs(rng, lo, hi, n=N):
    return _dirs(rng, n) * rng.uniform(lo, hi, size=(n, 1))


def rotation_vectors():
    """zone name -> rotation vectors (N, 3), for rodrigues."""
    rng = _rng(1)
    z = {}
    signs = np.array([[a, b, c] for a in (0.0, -0.0) for b in (0.0, -0.0) for c in (0.0, -0.0)])
    z["0"] = np.tile(signs, (8, 1))
    z["1e-301"] = _dirs(rng) * 1e-301
    z["1e-300"] = _dirs(rng) * 1e-300                                   # (its square underflows: fp64 sees |r| = 0 here too)
    z["1e-150"] = _rvecs(rng, 1e-150, 2e-150)                           # the first |r| whose square is a normal number
    z["1e-9"] = _rvecs(rng, 1e-9, 2e-9)
    z["1e-4"] = _rvecs(rng, 1e-4, 2e-4)
    z["1"] = _rvecs(rng, 0.5, 1.5)
    z["pi-1e-7"] = _dirs(rng) * (np.pi - rng.uniform(0, 1e-7, size=(N, 1)))
    z["pi"] = _dirs(rng) * np.pi
    z["3.2"] = _rvecs(rng, 3.15, 3.25)
    z["6.3"] = _rvecs(rng, 6.25, 6.35)
    return z


@functools.lru_cache(maxsize=None)
def rodrigues_zones():
    out = []
    with mpmath.workdps(DPS):
        for name, r in rotation_vectors().items():
            ref = np.array([_flat(mp_rotation([mpf(v) for v in ri])) for ri in r])
            th = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2])       # as fp64 sees it
            side = "<" if name in ("0", "1e-301", "1e-300") else ">"
            out.append(Zone(name, r, _by_ref(ref, [(slice(None), 1.0)]), [("th", th, TH_IDENTITY, side)]))
    return out


def _jr_and_g(r):
    """-> (Jr (9), R (9), G0 (9), G1 (9)) by central differences of the exact rotation: R^T dR/dr_j = [Jr e_j]x and
    G[c][i][j] = d(R e_c)_i / dr_j."""
    x = [mpf(v) for v in r]
    R = mp_rotation(x)
    D = mp_fd(lambda v: [e for row in mp_rotation(v) for e in row], x)              # D[3 i + c][j] = dR[i][c] / dr_j
    Jr = [[None] * 3 for _ in range(3)]
    for j in range(3):
        W = [[sum(R[k][a] * D[3 * k + b][j] for k in range(3)) for b in range(3)] for a in range(3)]       # R^T dR
        Jr[0][j], Jr[1][j], Jr[2][j] = (W[2][1] - W[1][2]) / 2, (W[0][2] - W[2][0]) / 2, (W[1][0] - W[0][1]) / 2
    G = [[[D[3 * i + c][j] for j in range(3)] for i in range(3)] for c in range(2)]
    return _flat(Jr), _flat(R), _flat(G[0]), _flat(G[1])


def jacobian_vectors():
    rng = _rng(2)
    z = {}
    for name, lo, hi in (("1e-6", 0.97e-6, 1.03e-6), ("0.9e-4", 0.85e-4, 0.95e-4), ("1.1e-4", 1.05e-4, 1.15e-4),
                         ("3e-4", 2.9e-4, 3.1e-4), ("1e-3", 0.97e-3, 1.03e-3), ("1e-2", 0.97e-2, 1.03e-2)):
        z[name] = _rvecs(rng, lo, hi)
    z["1"] = _rvecs(rng, 0.5, 1.5)
    z["pi-1e-7"] = _dirs(rng) * (np.pi - rng.uniform(0, 1e-7, size=(N, 1)))
    return z


@functools.lru_cache(maxsize=None)
def _jacobian_refs():
    with mpmath.workdps(DPS):
        return {name: (r, [np.array(t) for t in zip(*[_jr_and_g(ri) for ri in r])]) for name, r in jacobian_vectors().items()}


def _th2_side(name, r):
    th2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
    return [("th2", th2, TH2_SERIES, "<" if name in ("1e-6", "0.9e-4") else ">")]


@functools.lru_cache(maxsize=None)
def right_jacobian_zones():
    return [Zone(name, r, _by_ref(ref[0], [(slice(None), 1.0)]), _th2_side(name, r)) for name, (r, ref) in _jacobian_refs().items()]


@functools.lru_cache(maxsize=None)
def pose_basis_zones():
    """out = R (9), G[0] (9), G[1] (9); every entry of R and of G is of size 1."""
    return [Zone(name, r, _by_ref(np.concatenate(ref[1:], 1), [(slice(0, 9), 1.0), (slice(9, 27), 1.0)]), _th2_side(name, r))
            for name, (r, ref) in _jacobian_refs().items()]


@functools.lru_cache(maxsize=None)
def pose_columns_zones():
    """du (3), dv (3), mx, my, G (18) -> ju (6), jv (6); no branch: one zone of pixel-sized derivatives and board-sized points."""
    rng = _rng(3)
    x = np.concatenate([rng.normal(size=(N, 6)) * 300.0, rng.uniform(0.0, 0.1, size=(N, 2)), rng.normal(size=(N, 18))], 1)
    w = x.astype(LD)
    ref = np.zeros((N, 12), LD)
    for j in range(3):
        dX = [w[:, 6] * w[:, 8 + c * 3 + j] + w[:, 7] * w[:, 17 + c * 3 + j] for c in range(3)]
        ref[:, j] = sum(w[:, c] * dX[c] for c in range(3))
        ref[:, 6 + j] = sum(w[:, 3 + c] * dX[c] for c in range(3))
        ref[:, 3 + j], ref[:, 9 + j] = w[:, j], w[:, 3 + j]
    return [Zone("generic", x, _by_ref(ref, [([0, 1, 2, 6, 7, 8], None), ([3, 4, 5, 9, 10, 11], None)]))]


def _ld_rotation(r):
    return cx.rotation(np.asarray(r, np.float64))


def rvec_matrices():
    """zone name -> (matrices (n, 9) float64, kind): 'trip' = the formula arm, 'zero' and 'half' = the s < 1e-5 arms."""
    rng = _rng(4)
    z = {}

    def mats(rv):
        return np.array([cx.f64(_ld_rotation(r)).ravel() for r in rv])

    z["near identity s 1.1e-5..1e-3"] = (mats(_dirs(rng) * np.exp(rng.uniform(np.log(1.1e-5), np.log(1e-3), size=(N, 1)))), "trip")
    z["near half turn s 1.1e-5..1e-3"] = (mats(_dirs(rng) * (np.pi - np.exp(rng.uniform(np.log(1.1e-5), np.log(1e-3), size=(N, 1))))), "trip")
    z["generic"] = (mats(_rvecs(rng, 0.1, 3.0)), "trip")
    g = mats(_rvecs(rng, 0.1, 3.0))
    z["generic off by 1e-12"] = (g + rng.uniform(-1e-12, 1e-12, size=g.shape), "trip")
    z["s < 1e-5, c > 0"] = (mats(_dirs(rng) * rng.uniform(0, 0.9e-5, size=(N, 1))), "zero")
    # the half-turn arm: every sign pattern of the axis, axes with a zero component, and axes whose x is the smallest (the sign
    # fix-up); component sizes 0.2 / 0.5 / 0.84 apart, so that no comparison of |x|, |y|, |z| is a coin toss
    axes = []
    for perm in ((0.2, 0.5, 0.84), (0.5, 0.2, 0.84), (0.84, 0.5, 0.2), (0.5, 0.84, 0.2), (0.2, 0.84, 0.5), (0.84, 0.2, 0.5)):
        for sx in (1, -1):
            for sy in (1, -1):
                for sz in (1, -1):
                    axes.append((sx * perm[0], sy * perm[1], sz * perm[2]))
    for zero in range(3):
        for s1 in (1, -1):
            for s2 in (1, -1):
                a = [0.6 * s1, 0.8 * s2]
                a.insert(zero, 0.0)
                axes.append(tuple(a))
    axes += [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)]
    axes = np.array(axes)
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    z["s < 1e-5, c < 0"] = (mats(axes * (np.pi - rng.uniform(0, 0.9e-5, size=(len(axes), 1)))), "half")
    return z


def _rvec_definition_ld(R):
    """The s < 1e-5 arms of the matrix -> vector conversion (cvRodrigues2's, as the header states them), in the working precision."""
    R = np.asarray(R, np.float64).reshape(3, 3).astype(LD)
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    if c > 0:
        return np.zeros(3, LD)
    x = np.sqrt(max((R[0, 0] + 1) / 2, LD(0)))
    y = np.sqrt(max((R[1, 1] + 1) / 2, LD(0))) * (-1 if R[0, 1] < 0 else 1)
    z = np.sqrt(max((R[2, 2] + 1) / 2, LD(0))) * (-1 if R[0, 2] < 0 else 1)
    if abs(x) < abs(y) and abs(x) < abs(z) and ((R[1, 2] > 0) != (y * z > 0)):
        z = -z
    v = np.array([x, y, z], LD)
    return v * (LD(mpmath_pi_ld()) / np.sqrt(v @ v))


@functools.lru_cache(maxsize=None)
def mpmath_pi_ld():
    with mpmath.workdps(30):
        hi = float(mpmath.pi)
        return LD(hi) + LD(float(mpmath.pi - mpmath.mpf(hi)))


def _s_of(M):
    rx, ry, rz = M[:, 7] - M[:, 5], M[:, 2] - M[:, 6], M[:, 3] - M[:, 1]
    return np.sqrt((rx * rx + ry * ry + rz * rz) * 0.25)


@functools.lru_cache(maxsize=None)
def rvec_of_zones():
    out = []
    for name, (M, kind) in rvec_matrices().items():
        s = _s_of(M)
        c = (M[:, 0] + M[:, 4] + M[:, 8] - 1.0) * 0.5
        if kind == "trip":
            # the round trip through the exact rotation: max |R(rvec_of R) - R|, entries of size 1
            def measure(out_, iout=None, M=M):
                if not np.isfinite(out_).all():
                    return math.inf
                return max(float(np.abs(_ld_rotation(r).ravel() - M[i].astype(LD)).max()) for i, r in enumerate(out_))
            out.append(Zone(name, M, measure, [("s", s, S_SMALL, ">")]))
        elif kind == "zero":
            assert (c > 0).all()
            out.append(Zone(name, M, lambda out_, iout=None: 0.0 if not np.asarray(out_).any() else math.inf,
                            [("s", s, S_SMALL, "<")], "exactly zero"))
        else:
            assert (c < 0).all()
            ref = np.array([_rvec_definition_ld(m) for m in M])
            out.append(Zone(name, M, _by_ref(ref, [(slice(None), math.pi)]), [("s", s, S_SMALL, "<")]))
    return out


# ------------------------------------------------------------------------------------------------ the pinhole model

K_PIN = cx.K_EDGE
NEG_LENS = np.array([-0.5, 0.0, 1e-3, -1e-3])          # 1 + k1 r^2 changes sign at r^2 = 2: undistort's icdist < 0 arm
PIN_MODELS = dict(cx.MODELS)


def cam12(K, dist):
    return np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], cx.dist8(dist)]


def _pin_points(rng, zone):
    """Camera-frame points q (N, 3) of a zone -> q"""
    if zone == "axis":                       # on the optical axis, and within 1e-9 of it
        q = np.zeros((N, 3))
        q[N // 2:, :2] = rng.uniform(-1e-9, 1e-9, size=(N - N // 2, 2))
        q[:, 2] = rng.uniform(0.1, 2.0, size=N)
    elif zone == "field":                    # out to the field's edge: |x|, |y| up to 0.5 (157 px of 310)
        z = rng.uniform(0.1, 2.0, size=N)
        q = np.c_[rng.uniform(-0.5, 0.5, size=N) * z, rng.uniform(-0.5, 0.5, size=N) * z, z]
    elif zone == "edge":                     # on the edge itself
        z = rng.uniform(0.1, 2.0, size=N)
        ang = rng.uniform(0, 2 * np.pi, size=N)
        q = np.c_[0.5 * np.cos(ang) * z, 0.5 * np.sin(ang) * z, z]
    elif zone == "qz 1e-6":
        z = np.full(N, 1e-6)
        q = np.c_[rng.uniform(-0.5, 0.5, size=N) * z, rng.uniform(-0.5, 0.5, size=N) * z, z]
    else:
        raise ValueError(zone)
    return q


def _pin_project_ref(cam, q, u, v):
    """-> ru, rv, du (3), dv (3), x, y, xd, yd in mpmath, the derivative by central differences in q."""
    c = [mpf(t) for t in cam]

    def pix(qq):
        xd, yd = mp_pinhole(qq[0] / qq[2], qq[1] / qq[2], c[4:])
        return [c[0] * xd + c[2], c[1] * yd + c[3]]

    qq = [mpf(t) for t in q]
    p = pix(qq)
    J = mp_fd(pix, qq, mpmath.mpf(10) ** -20 * qq[2])
    x, y = qq[0] / qq[2], qq[1] / qq[2]
    xd, yd = mp_pinhole(x, y, c[4:])
    return [float(t) for t in [p[0] - mpf(u), p[1] - mpf(v)] + J[0] + J[1] + [x, y, xd, yd]], float(max(abs(p[0]), abs(p[1])))


@functools.lru_cache(maxsize=None)
def project_zones():
    """in = camera (12), q (3), u, v; out = ru, rv, du (3), dv (3), x, y, xd, yd.  The residuals are scaled by the pixel
    coordinates they are differences of, the derivatives and the normalised points by their own largest entry in the zone."""
    out = []
    with mpmath.workdps(DPS):
        for mi, (model, dist) in enumerate(PIN_MODELS.items()):
            cam = cam12(K_PIN, dist)
            for zi, zone in enumerate(("axis", "field", "edge", "qz 1e-6")):
                rng = _rng(5, mi, zi)
                q = _pin_points(rng, zone)
                uv = rng.uniform(0, 320, size=(N, 2))
                refs = [_pin_project_ref(cam, q[i], uv[i, 0], uv[i, 1]) for i in range(N)]
                ref = np.array([r[0] for r in refs])
                pix = max(max(r[1] for r in refs), 320.0)
                x = np.c_[np.tile(cam, (N, 1)), q, uv]
                groups = [(slice(0, 2), pix), (slice(2, 8), None), (slice(8, 12), max(float(np.abs(ref[:, 8:12]).max()), 1e-9))]
                out.append(Zone(f"dist {model} / {zone}", x, _by_ref(ref, groups), [("qz", q[:, 2], 0.0, ">")]))
    return out


def behind_points():
    """q with q_z <= 0: zero, minus zero, negative, -inf and NaN (NaN is not > 0 either)."""
    rng = _rng(6)
    q = np.c_[rng.normal(size=(N, 2)), -np.abs(rng.normal(size=N))]
    q[:8, 2] = [0.0, -0.0, -1e-300, -1e300, -np.inf, np.nan, -5e-324, 0.0]
    return q


def _undistort_steps(cam, u, v, rounds=5):
    """The definition: five fixed-point steps from (x0, y0), given up (x0, y0 kept) once icdist < 0 -> (x, y, every icdist
    met), in mpmath."""
    c = [mpf(t) for t in cam]
    k = c[4:]
    x0, y0 = (mpf(u) - c[2]) / c[0], (mpf(v) - c[3]) / c[1]
    x, y, seen = x0, y0, []
    if not any(float(t) != 0.0 for t in k):
        return x0, y0, seen
    for _ in range(rounds):
        r2 = x * x + y * y
        ic = (1 + k[5] * r2 + k[6] * r2 ** 2 + k[7] * r2 ** 3) / (1 + k[0] * r2 + k[1] * r2 ** 2 + k[4] * r2 ** 3)
        seen.append(ic)
        if ic < 0:
            return x0, y0, seen
        dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
        dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
        x, y = (x0 - dx) * ic, (y0 - dy) * ic
    return x, y, seen


# undistort's true inverse where five steps converge.  With S = the sum of the |radial coefficients| (k1 k2 k3 k4 k5 k6) and P the
# larger |tangential| one, on |x| <= R = R_CONV the step's map x -> (x0 - dx(x)) icdist(x) has a Lipschitz constant of at most
# q = 3 S R^2 + 6 P R (|x0| |d icdist| <= 2 S R^2 to first order, |d dx| <= 6 P R; 3 S R^2 leaves room for the higher orders), and
# the start x0 is at most d0 = S R^3 + 3 P R^2 from the true inverse, so five steps end within q^5 d0 of it: 4e-12 for the
# coefficient sets of camera_exact.MODELS, 9e-11 for NEG_LENS.
R_CONV = 0.15


def conv_bound(dist):
    k = cx.dist8(dist)
    S, P = float(np.abs(k[[0, 1, 4, 5, 6, 7]]).sum()), float(np.abs(k[2:4]).max())
    return (3 * S * R_CONV ** 2 + 6 * P * R_CONV) ** 5 * (S * R_CONV ** 3 + 3 * P * R_CONV ** 2)


@functools.lru_cache(maxsize=None)
def undistort_zones():
    """in = camera (12), u, v; out = x, y.  Zones: each coefficient set at the centre (r <= 0.15, where the five steps have
    converged: ``expect`` holds the true inverse), over the field, and the lens whose icdist turns negative."""
    out = []
    lenses = list(PIN_MODELS.items()) + [("neg", NEG_LENS)]
    with mpmath.workdps(DPS):
        for mi, (model, dist) in enumerate(lenses):
            cam = cam12(K_PIN, dist)
            for zi, zone in enumerate(("centre", "field") + (("icdist < 0",) if model == "neg" else ())):
                rng = _rng(7, mi, zi)
                ang = rng.uniform(0, 2 * np.pi, size=N)
                rad = {"centre": rng.uniform(0, R_CONV * 0.95, size=N), "field": rng.uniform(0.2, 0.6, size=N),
                       "icdist < 0": rng.uniform(1.6, 2.0, size=N)}[zone]
                if zone == "centre":
                    rad[0] = 0.0
                # the true normalised point; its pixel through the exact model, as float64
                xt, yt = rad * np.cos(ang), rad * np.sin(ang)
                if zone == "icdist < 0":
                    pix = np.c_[cam[0] * xt + cam[2], cam[1] * yt + cam[3]]               # (here (xt, yt) is x0 itself)
                else:
                    pix = cx.f64(cx.distort(cx._w(xt), cx._w(yt), K_PIN, cx.dist8(dist)))
                steps = [_undistort_steps(cam, *p) for p in pix]
                ref = np.array([[float(s[0]), float(s[1])] for s in steps])
                ics = np.array([float(t) for s in steps for t in s[2]])
                sides = []
                if zone == "icdist < 0":
                    first = np.array([float(s[2][0]) for s in steps])
                    sides = [("-icdist", -first, 0.01, ">")]
                elif ics.size:
                    sides = [("icdist", ics, 0.01, ">")]
                x = np.c_[np.tile(cam, (N, 1)), pix]
                scale = max(float(np.abs(ref).max()), 0.1)
                expect = (np.c_[xt, yt], conv_bound(dist)) if zone == "centre" else None
                out.append(Zone(f"dist {model} / {zone}", x, _by_ref(ref, [(slice(None), scale)]), sides, expect))
    return out


# ------------------------------------------------------------------------------------------------ the fisheye model

K_FISH = fe.camera(400.0, 380.0, off=(3.5, -2.25))
K_FISH0 = np.array([[400.0, 0, 0], [0, 380.0, 0], [0, 0, 1.0]])             # principal point at 0: pixels resolve theta_d = 1e-8
FISH_LENSES = {"K_LENS": fe.K_LENS, "K_ZERO": fe.K_ZERO, "k1 < 0": np.array([-0.05, 0.01, 0.0, 0.0])}
SMALL_R = 1e-4
SMALL_THETA_D = 1e-8
FISH_R = [("r = 0", None, "<"), ("r 1e-12", (1e-12, 2e-12), "<"), ("r 0.9e-4", (0.85e-4, 0.95e-4), "<"),
          ("r 1.1e-4", (1.05e-4, 1.15e-4), ">"), ("r 1e-2", (1e-2, 2e-2), ">"), ("r 1", (0.5, 2.0), ">"),
          ("r to 89.9 deg", (5.0, math.tan(math.radians(89.9))), ">")]


def _fish_ab(rng, span):
    if span is None:
        return np.zeros((N, 2))
    r = np.exp(rng.uniform(np.log(span[0]), np.log(span[1]), size=N))
    r[0], r[1] = span
    ang = rng.uniform(0, 2 * np.pi, size=N)
    return np.c_[r * np.cos(ang), r * np.sin(ang)]


def _fish_distort_ref(k, a, b):
    """-> xd, yd, tt, t2, dxa, dxb, dyb (dyd/da = dxb by the model's symmetry; tt = theta / r -> 1 at r = 0)."""
    kk = [mpf(t) for t in k]
    ab = [mpf(a), mpf(b)]
    xd, yd = mp_fisheye(ab[0], ab[1], kk)
    J = mp_fd(lambda v: mp_fisheye(v[0], v[1], kk), ab)
    r = mpmath.sqrt(ab[0] ** 2 + ab[1] ** 2)
    th = mpmath.atan(r)
    return [float(t) for t in (xd, yd, th / r if r != 0 else mpmath.mpf(1), th * th, J[0][0], J[0][1], J[1][1])]


@functools.lru_cache(maxsize=None)
def fisheye_distort_zones():
    """in = k (4), a, b; out = xd, yd, tt, t2, dxa, dxb, dyb.  (xd, yd) are scaled by their largest entry in the zone, tt and the
    derivatives by 1 (they are 1 on the axis), t2 by its largest entry."""
    out = []
    with mpmath.workdps(DPS):
        for li, (lens, k) in enumerate(FISH_LENSES.items()):
            for zi, (zone, span, side) in enumerate(FISH_R):
                ab = _fish_ab(_rng(8, li, zi), span)
                ref = np.array([_fish_distort_ref(k, *p) for p in ab])
                r2 = ab[:, 0] * ab[:, 0] + ab[:, 1] * ab[:, 1]
                tiny = 1e-300
                groups = [(slice(0, 2), max(float(np.abs(ref[:, :2]).max()), tiny)), ([2, 4, 5, 6], 1.0),
                          ([3], max(float(ref[:, 3].max()), tiny))]
                out.append(Zone(f"{lens} / {zone}", np.c_[np.tile(k, (N, 1)), ab], _by_ref(ref, groups),
                                [("r", np.sqrt(r2), SMALL_R, side)]))
    return out


def cam8(K, k):
    return np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], np.asarray(k, np.float64)]


@functools.lru_cache(maxsize=None)
def fisheye_project_zones():
    """in = camera (8), q (3), u, v; out = ru, rv, du (3), dv (3), a, b, xd, yd, tt, t2.  One zone per lens over the field
    (r from 1e-3 to 10, depths 0.05 to 2), and one at q_z = 1e-6."""
    out = []
    with mpmath.workdps(DPS):
        for li, (lens, k) in enumerate(FISH_LENSES.items()):
            cam = cam8(K_FISH, k)
            c = [mpf(t) for t in cam]

            def pix(qq):
                xd, yd = mp_fisheye(qq[0] / qq[2], qq[1] / qq[2], c[4:])
                return [c[0] * xd + c[2], c[1] * yd + c[3]]

            for zi, zone in enumerate(("field", "qz 1e-6")):
                rng = _rng(9, li, zi)
                ab = _fish_ab(rng, (1e-3, 10.0))
                z = rng.uniform(0.05, 2.0, size=N) if zone == "field" else np.full(N, 1e-6)
                q = np.c_[ab * z[:, None], z]
                uv = rng.uniform(0, 640, size=(N, 2))
                ref = []
                for i in range(N):
                    qq = [mpf(t) for t in q[i]]
                    p = pix(qq)
                    J = mp_fd(pix, qq, mpmath.mpf(10) ** -20 * qq[2])
                    a_, b_ = qq[0] / qq[2], qq[1] / qq[2]
                    xd, yd = mp_fisheye(a_, b_, c[4:])
                    r = mpmath.sqrt(a_ * a_ + b_ * b_)
                    th = mpmath.atan(r)
                    ref.append([float(t) for t in [p[0] - mpf(uv[i, 0]), p[1] - mpf(uv[i, 1])] + J[0] + J[1] +
                                [a_, b_, xd, yd, th / r, th * th]])
                ref = np.array(ref)
                groups = [(slice(0, 2), 1000.0), (slice(2, 8), None), (slice(8, 10), None), (slice(10, 12), None), ([12], 1.0),
                          ([13], None)]
                rr = np.sqrt((q[:, 0] / q[:, 2]) ** 2 + (q[:, 1] / q[:, 2]) ** 2)
                out.append(Zone(f"{lens} / {zone}", np.c_[np.tile(cam, (N, 1)), q, uv], _by_ref(ref, groups),
                                [("qz", q[:, 2], 0.0, ">"), ("r", rr, SMALL_R, ">")]))
    return out


def _theta_of(thd, k):
    """The root theta of theta (1 + k1 theta^2 + ...) = theta_d nearest the start theta_d, by Newton in mpmath, or None."""
    f = lambda t: t * (1 + k[0] * t ** 2 + k[1] * t ** 4 + k[2] * t ** 6 + k[3] * t ** 8) - thd
    try:
        return mpmath.findroot(f, thd, tol=mpmath.mpf(10) ** -40, maxsteps=200)
    except (ValueError, ZeroDivisionError):
        return None


def _thd_of(th, k):
    th = np.asarray(th, LD)
    t2 = th * th
    return th * (1 + t2 * (LD(k[0]) + t2 * (LD(k[1]) + t2 * (LD(k[2]) + t2 * LD(k[3])))))


@functools.lru_cache(maxsize=None)
def fisheye_undistort_zones():
    """in = camera (8), u, v; out = x, y and the inside flag.  Zones by theta_d (the switch kFisheyeSmallThetaD) and by theta up
    to pi / 2 - 1e-6; the verdict is asked only where it is no coin toss: theta <= pi / 2 - 1e-6 inside, theta >= pi / 2 + 1e-6
    outside.  ``expect`` = the verdict."""
    out = []
    half = math.pi / 2
    spans = [("theta_d = 0", None, "<"), ("theta_d 0.9e-8", (0.85e-8, 0.95e-8), "<"), ("theta_d 1.1e-8", (1.05e-8, 1.15e-8), ">"),
             ("theta 1e-4", (1e-4, 2e-4), ">"), ("theta 0.1 to 1.5", (0.1, 1.5), ">"),
             ("theta to pi/2 - 1e-6", (1.5, half - 1e-6), ">"), ("outside", (half + 1e-6, 1.8), ">")]      # (theta_d stays increasing to 1.8 on every lens here)
    with mpmath.workdps(DPS):
        for li, (lens, k) in enumerate(FISH_LENSES.items()):
            kk = [mpf(t) for t in k]
            for zi, (zone, span, side) in enumerate(spans):
                rng = _rng(10, li, zi)
                K = K_FISH0 if "theta_d" in zone else K_FISH
                cam = cam8(K, k)
                ang = rng.uniform(0, 2 * np.pi, size=N)
                if span is None:
                    thd = np.zeros(N)
                elif "theta_d" in zone:
                    thd = rng.uniform(*span, size=N)
                else:                                         # theta is placed, theta_d follows from it
                    if "pi/2" in zone:                        # crowd the upper end: pi/2 - 1e-6 .. pi/2 - 0.07
                        th = half - np.exp(rng.uniform(np.log(1e-6), np.log(0.07), size=N))
                        th[0] = half - 1e-6
                    else:
                        th = rng.uniform(*span, size=N)
                        if zone == "outside":
                            th[0] = half + 1e-6
                    thd = cx.f64(_thd_of(th, k))
                pix = np.c_[cam[0] * thd * np.cos(ang) + cam[2], cam[1] * thd * np.sin(ang) + cam[3]]
                # what the block sees: theta_d of the float64 pixel
                c = [mpf(t) for t in cam]
                ref, verdict, thd_seen = [], [], []
                for p in pix:
                    xp, yp = (mpf(p[0]) - c[2]) / c[0], (mpf(p[1]) - c[3]) / c[1]
                    td = mpmath.sqrt(xp * xp + yp * yp)
                    thd_seen.append(float(td))
                    th_ = _theta_of(td, kk) if td != 0 else mpmath.mpf(0)
                    if zone == "outside":
                        assert th_ is None or th_ >= half + 0.999e-6, (lens, float(td), th_)
                        ref.append([math.nan, math.nan])
                        verdict.append(0)
                        continue
                    assert th_ is not None and 0 <= th_ <= half - mpmath.mpf(10) ** -6 * mpmath.mpf("0.999"), (lens, zone, th_)
                    s = mpmath.tan(th_) / td if td != 0 else mpmath.mpf(1)
                    ref.append([float(xp * s), float(yp * s)])
                    verdict.append(1)
                ref = np.array(ref)
                x = np.c_[np.tile(cam, (N, 1)), pix]
                sides = [("theta_d", np.array(thd_seen), SMALL_THETA_D, side)]
                if zone == "outside":
                    measure = lambda out_, iout=None: 0.0 if np.isnan(np.asarray(out_)).all() else math.inf
                else:
                    measure = _by_ref(ref, [(slice(None), max(float(np.abs(ref).max()), 1e-300))])
                out.append(Zone(f"{lens} / {zone}", x, measure, sides, np.array(verdict)))
    return out


# ------------------------------------------------------------------------------------------------ small matrices

def _sym(n, rng, w):
    """Q diag(w) Q^T with a random orthogonal Q, symmetrised, float64."""
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    A = (Q * w) @ Q.T
    return (A + A.T) / 2


def pack(A):
    n = A.shape[0]
    return np.array([A[i, j] for i in range(n) for j in range(i, n)])


def unpack(p, n):
    A = np.zeros((n, n), np.asarray(p).dtype)
    e = 0
    for i in range(n):
        for j in range(i, n):
            A[i, j] = A[j, i] = p[e]
            e += 1
    return A


def dlt_normal_matrix(obj_xy, mn):
    """The 9 x 9 DLT normal matrix of Hartley-normalised correspondences, float64 (plain numpy; an input for jacobi<9, 1>)."""
    a, b = obj_xy - obj_xy.mean(0), mn - mn.mean(0)
    a = a * (math.sqrt(2) / np.sqrt((a ** 2).sum(1)).mean())
    b = b * (math.sqrt(2) / np.sqrt((b ** 2).sum(1)).mean())
    M = np.zeros((9, 9))
    for (X, Y), (u, v) in zip(a, b):
        r1 = np.array([X, Y, 1, 0, 0, 0, -u * X, -u * Y, -u])
        r2 = np.array([0, 0, 0, X, Y, 1, -v * X, -v * Y, -v])
        M += np.outer(r1, r1) + np.outer(r2, r2)
    return M


def symmetric_cases(n, count):
    """zone name -> (count, n, n) symmetric float64 matrices."""
    rng = _rng(11, n)
    z = {}
    z["diagonal"] = np.array([np.diag(rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3)) for _ in range(count)])
    z["generic"] = np.array([_sym(n, rng, rng.normal(size=n)) for _ in range(count)])
    rep = []
    for _ in range(count):
        w = rng.uniform(0.5, 2.0, size=n)
        w[1] = w[0]
        if n > 3:
            w[4] = w[3] = w[2]
        rep.append(_sym(n, rng, w))
    z["repeated eigenvalue"] = np.array(rep)
    z["1e-30 to 1e30"] = np.array([(lambda d, A: A * np.outer(d, d))(10.0 ** rng.uniform(-15, 15, size=n), _sym(n, rng, rng.uniform(0.5, 2, size=n)))
                                   for _ in range(count)])
    deficient = []
    for _ in range(count):
        B = rng.integers(-3, 4, size=(n, n - 1 - (n > 3))).astype(np.float64)           # small integers: B B^T is exact, rank < n
        deficient.append(B @ B.T)
    z["exactly rank deficient"] = np.array(deficient)
    huge = []
    for _ in range(count):
        A = _sym(n, rng, rng.uniform(0.5, 2.0, size=n))
        A[0, 1] = A[1, 0] = 1e-200 * rng.uniform(1, 2)                                # (aqq - app) / (2 apq) ~ 1e200
        A[1, 1] += 1.0
        huge.append(A)
    z["huge (aqq - app) / 2 apq"] = np.array(huge)
    zero = []
    for _ in range(count):
        A = _sym(n, rng, rng.uniform(0.5, 2.0, size=n))
        A[0, 1] = A[1, 0] = 0.0
        A[0, n - 1] = A[n - 1, 0] = 0.0
        zero.append(A)
    z["off-diagonal exactly zero"] = np.array(zero)
    if n == 9:                                                           # DLT normal matrices of noise-free boards
        dlt = []
        for i, f in enumerate(cx.grid()):
            if f.sigma == 0.0 and f.model == "none" and f.board == cx.BOARDS[3] and len(dlt) < count:
                obj, img, _ = cx.pool_rows(f)
                mn = (img - np.array([K_PIN[0, 2], K_PIN[1, 2]])) / np.array([K_PIN[0, 0], K_PIN[1, 1]])
                dlt.append(dlt_normal_matrix(obj[:, :2].astype(np.float64), mn))
        z["DLT normal matrices"] = np.array(dlt)
    return z


def eigen_measures(A, w, V, w_ref):
    """-> (|V^T V - I|, |A V - V diag w| / |A|, |sorted w - reference| / |A|), max norms."""
    A, V, w = A.astype(LD), np.asarray(V).astype(LD), np.asarray(w).astype(LD)
    na = float(np.abs(A).max()) or 1.0
    orth = float(np.abs(V.T @ V - np.eye(len(w))).max())
    resid = float(np.abs(A @ V - V * w).max()) / na
    eig = float(np.abs(np.sort(w) - w_ref).max()) / na
    if not (np.isfinite(orth) and np.isfinite(resid) and np.isfinite(eig)):
        return math.inf, math.inf, math.inf
    return orth, resid, eig


@functools.lru_cache(maxsize=None)
def eigen_reference(n, count):
    """zone -> (matrices, sorted eigenvalues by mpmath.eigsy in 40 digits, as long double)."""
    out = {}
    with mpmath.workdps(40):
        for name, As in symmetric_cases(n, count).items():
            ws = []
            for A in As:
                E = mpmath.eigsy(mpmath.matrix([[mpf(v) for v in row] for row in A]), eigvals_only=True)
                ws.append(np.sort(np.array([cx.LD(float(e)) + cx.LD(float(e - mpmath.mpf(float(e)))) for e in E])))
            out[name] = (As, np.array(ws))
    return out


JACOBI3_COUNT, JACOBI9_COUNT = 64, 24         # 9 x 9: 24 matrices a zone, each run by all 64 lanes of a workgroup


def jacobi_gap(As, w_ref, ws, Vs):
    """The zone's three measures over its matrices -> (orthogonality, residual, eigenvalues)."""
    m = np.array([eigen_measures(A, w, V, wr) for A, w, V, wr in zip(As, ws, Vs, w_ref)])
    return tuple(m.max(0))


def polar_matrices():
    rng = _rng(12)
    z = {}
    z["random"] = rng.normal(size=(N, 9))
    rot = np.array([cx.f64(_ld_rotation(r)).ravel() for r in _rvecs(rng, 0.0, 3.1)])
    z["near rotations"] = rot + rng.uniform(-1e-3, 1e-3, size=rot.shape)
    neg = rot.copy()
    neg[:, [2, 5, 8]] *= -1.0                                       # third column flipped: det = -1
    z["det < 0"] = neg + rng.uniform(-1e-3, 1e-3, size=rot.shape)
    z["scaled 1e-8"] = rng.normal(size=(N, 9)) * 1e-8
    z["scaled 1e8"] = rng.normal(size=(N, 9)) * 1e8
    return z


def singular_matrices():
    """A zero column (each position), two zero columns, the zero matrix: M^T M has an exact zero eigenvalue -> false."""
    rng = _rng(13)
    M = rng.normal(size=(N, 3, 3))
    for i in range(N):
        kind = i % 7
        if kind < 3:
            M[i][:, kind] = 0.0
        elif kind < 6:
            M[i][:, [(kind - 3), (kind - 2) % 3]] = 0.0
        else:
            M[i] = 0.0
    return M.reshape(N, 9)


def _mp_polar(M):
    """M (M^T M)^-1/2 in mpmath -> 9 floats, and the condition number of M."""
    A = mpmath.matrix([[mpf(M[3 * i + j]) for j in range(3)] for i in range(3)])
    E, Q = mpmath.eigsy(A.T * A)
    P = Q * mpmath.diag([1 / mpmath.sqrt(e) for e in E]) * Q.T
    U = A * P
    return [float(U[i, j]) for i in range(3) for j in range(3)]


@functools.lru_cache(maxsize=None)
def polar_factor_zones():
    """in = M (9); out = Q (9).  measure = max(|Q - Q_ref|, |Q^T Q - I|), entries of size 1."""
    out = []
    with mpmath.workdps(DPS):
        for name, Ms in polar_matrices().items():
            ref = np.array([_mp_polar(M) for M in Ms])

            def measure(out_, iout=None, ref=ref):
                Q = np.asarray(out_).reshape(-1, 3, 3).astype(LD)
                if not np.isfinite(np.asarray(out_)).all():
                    return math.inf
                orth = max(float(np.abs(q.T @ q - np.eye(3)).max()) for q in Q)
                return max(orth, float(np.abs(Q.reshape(-1, 9) - ref).max()))
            out.append(Zone(name, Ms, measure))
    return out


CHOLESKY_CONDS = (1e2, 1e8, 1e12)
CHOLESKY_SCALES = (1.0, 1.001, 2.0)


def _mp_solve(A, b):
    return [float(v) for v in mpmath.lu_solve(mpmath.matrix([[mpf(v) for v in row] for row in A]), mpmath.matrix([mpf(v) for v in b]))]


@functools.lru_cache(maxsize=None)
def cholesky_zones():
    """in = packed JtJ (21), Jtr (6), scale; out = x (6).  The reference solves (A with its diagonal times scale) x = b in
    mpmath; the gap is relative to |x|.  ``expect`` = the L of that matrix by mpmath, packed, for cholesky_factor."""
    out = []
    with mpmath.workdps(DPS):
        for ci, cond in enumerate(CHOLESKY_CONDS):
            rng = _rng(14, ci)
            xs, refs, Ls = [], [], []
            for i in range(N):
                w = np.exp(np.linspace(0, np.log(cond), 6))
                A = _sym(6, rng, w)
                b = rng.normal(size=6)
                scale = CHOLESKY_SCALES[i % 3]
                Am = mpmath.matrix([[mpf(v) for v in row] for row in A])
                for d in range(6):
                    Am[d, d] = Am[d, d] * mpf(scale)
                x = mpmath.lu_solve(Am, mpmath.matrix([mpf(v) for v in b]))
                L = mpmath.cholesky(Am)
                xs.append(np.r_[pack(A), b, scale])
                refs.append([float(v) for v in x])
                Ls.append([float(L[i_, j_]) for j_ in range(6) for i_ in range(j_, 6)])
            ref = np.array(refs)

            def measure(out_, iout=None, ref=ref):
                o = np.asarray(out_).astype(LD)
                if not np.isfinite(np.asarray(out_)).all():
                    return math.inf
                return float((np.abs(o - ref).max(1) / np.abs(ref).max(1)).max())
            out.append(Zone(f"cond {cond:g}", np.array(xs), measure, (), np.array(Ls)))
    return out


def lower_packed_to_pk(Lcol):
    """cholesky_zones' ``expect`` (L by columns: L[j..5][j]) -> the header's packed order pk<6>(i, j) over i <= j slots."""
    L = np.zeros((6, 6))
    e = 0
    for j in range(6):
        for i in range(j, 6):
            L[i, j] = L[j, i] = Lcol[e]
            e += 1
    return pack(L)


def cholesky_refusals():
    """packed A (21), b (6), scale -> must return false: a zero pivot, a negative pivot (first, middle, last), a NaN entry, and
    scale = 0, scale < 0."""
    rng = _rng(15)
    rows = []
    for i in range(N):
        A = _sym(6, rng, rng.uniform(1, 3, size=6))
        scale = 1.0
        kind = i % 8
        if kind == 0:
            A[0, 0] = 0.0
        elif kind == 1:
            A[0, 0] = -1.0
        elif kind == 2:
            A[3, 3] = -5.0
        elif kind == 3:
            A[5, 5] = -5.0
        elif kind == 4:
            j, k = rng.integers(0, 6, size=2)
            A[j, k] = A[k, j] = np.nan
        elif kind == 5:
            scale = 0.0
        elif kind == 6:
            scale = -1.0
        else:                                   # rows 0 and 1 equal: the second pivot is exactly zero
            A = np.diag(np.arange(1.0, 7.0))
            A[1, 1] = A[0, 0] = A[0, 1] = A[1, 0] = 4.0
        rows.append(np.r_[pack(A), rng.normal(size=6), scale])
    return np.array(rows)


# ------------------------------------------------------------------------------------------------ four points

def quadruples():
    """zone -> (board points (n, 4, 2), image points (n, 4, 2)): general ones (a random homography of a convex quadrilateral)
    and ones with three board points nearly on a line (height 1e-3 of the base)."""
    rng = _rng(16)
    z = {}
    for name in ("general", "three nearly on a line"):
        objs, imgs = [], []
        while len(objs) < N:
            if name == "general":
                obj = np.array([[0.0, 0], [1, 0], [1, 1], [0, 1]]) * 0.1 + rng.uniform(-0.02, 0.02, size=(4, 2)) + rng.uniform(0, 0.3, size=2)
            else:
                obj = np.array([[0.0, 0], [0.05, 1e-4 * rng.uniform(0.5, 1)], [0.1, 0], [0.03, 0.08]]) + rng.uniform(0, 0.3, size=2)
            H = np.eye(3) + rng.normal(size=(3, 3)) * 0.2
            H[2, :2] *= 0.5
            w = np.c_[obj, np.ones(4)] @ H.T
            if (w[:, 2] < 0.3).any():
                continue
            objs.append(obj)
            imgs.append(w[:, :2] / w[:, 2:])
        z[name] = (np.array(objs), np.array(imgs))
    return z


def _mp_homography4(obj, img):
    """The homography through four correspondences by the eight-equation solve (h33 = 1), board points centred -> H (9)."""
    mc = [sum(mpf(o[c]) for o in obj) / 4 for c in range(2)]
    A, b = mpmath.matrix(8, 8), mpmath.matrix(8, 1)
    for i in range(4):
        X, Y, u, v = mpf(obj[i][0]) - mc[0], mpf(obj[i][1]) - mc[1], mpf(img[i][0]), mpf(img[i][1])
        A[2 * i, 0], A[2 * i, 1], A[2 * i, 2], A[2 * i, 6], A[2 * i, 7] = X, Y, 1, -u * X, -u * Y
        A[2 * i + 1, 3], A[2 * i + 1, 4], A[2 * i + 1, 5], A[2 * i + 1, 6], A[2 * i + 1, 7] = X, Y, 1, -v * X, -v * Y
        b[2 * i], b[2 * i + 1] = u, v
    h = mpmath.lu_solve(A, b)
    return [float(v) for v in h] + [1.0], [float(v) for v in mc]


@functools.lru_cache(maxsize=None)
def homography4_zones():
    """in = mx (4), my (4), x (4), y (4); out = H (9), mcx, mcy.  H is scaled by its largest entry, the centroid by its own."""
    out = []
    with mpmath.workdps(DPS):
        for name, (objs, imgs) in quadruples().items():
            refs = [_mp_homography4(o, m) for o, m in zip(objs, imgs)]
            ref = np.array([r[0] + r[1] for r in refs])
            x = np.c_[objs[:, :, 0], objs[:, :, 1], imgs[:, :, 0], imgs[:, :, 1]]

            def measure(out_, iout=None, ref=ref):
                o = np.asarray(out_).astype(LD)
                if not np.isfinite(np.asarray(out_)).all():
                    return math.inf
                gh = (np.abs(o[:, :9] - ref[:, :9]).max(1) / np.abs(ref[:, :9]).max(1)).max()
                gc = (np.abs(o[:, 9:] - ref[:, 9:]).max(1) / np.abs(ref[:, 9:]).max(1)).max()
                return float(max(gh, gc))
            out.append(Zone(name, x, measure))
    return out


@functools.lru_cache(maxsize=None)
def adjugate_zones():
    """adjugate (9 -> 9) against the cofactors in the working precision, scaled by |m|^2; projective_basis (x (4), y (4) -> 9)
    against its definition A = [p1 p2 p3] diag(adj([p1 p2 p3]) p4) in the working precision, scaled by its largest entry."""
    rng = _rng(17)
    m = rng.normal(size=(N, 9)) * 10.0 ** rng.uniform(-3, 3, size=(N, 1))
    w = m.astype(LD).reshape(N, 3, 3)
    adj = np.array([[[(-1) ** (i + j) * _minor(a, j, i) for j in range(3)] for i in range(3)] for a in w]).reshape(N, 9)
    scale = (np.abs(m).max(1) ** 2).astype(LD)
    za = Zone("generic", m, lambda out_, iout=None: float((np.abs(np.asarray(out_).astype(LD) - adj).max(1) / scale).max()))
    objs = np.concatenate([v[1] for v in quadruples().values()])
    x = np.c_[objs[:, :, 0], objs[:, :, 1]]
    ref = []
    for p in objs.astype(LD):
        mm = np.array([[p[0, 0], p[1, 0], p[2, 0]], [p[0, 1], p[1, 1], p[2, 1]], [LD(1), LD(1), LD(1)]])
        a = np.array([[(-1) ** (i + j) * _minor(mm, j, i) for j in range(3)] for i in range(3)])
        lam = a @ np.array([p[3, 0], p[3, 1], LD(1)])
        ref.append((mm * lam).ravel())
    ref = np.array(ref)
    zp = Zone("image quadruples", x, lambda out_, iout=None: float((np.abs(np.asarray(out_).astype(LD) - ref).max(1) /
                                                                    np.abs(ref).max(1)).max()))
    return za, zp


def _minor(a, i, j):
    r = [k for k in range(3) if k != i]
    c = [k for k in range(3) if k != j]
    return a[r[0], c[0]] * a[r[1], c[1]] - a[r[0], c[1]] * a[r[1], c[0]]


# ------------------------------------------------------------------------------------------------ reductions

def butterfly(a):
    """wave_sum restated: a (64, NV) float64 -> every lane's sums (64, NV); m = 32, 16, ..., 1: a[l] += a[l ^ m]."""
    a = np.array(a, np.float64)
    lanes = np.arange(64)
    with np.errstate(all="ignore"):
        m = 32
        while m >= 1:
            a = a + a[lanes ^ m]
            m >>= 1
    return a


def tree(s):
    """block_tree restated: s (THREADS, NV) -> the totals s[0]; h = THREADS / 2, ..., 1: s[t] += s[t + h] for t < h."""
    s = np.array(s, np.float64)
    with np.errstate(all="ignore"):
        h = s.shape[0] // 2
        while h >= 1:
            s[:h] = s[:h] + s[h:2 * h]
            h //= 2
    return s[0]


def reduction_inputs(lanes, nv, count):
    """(count, lanes, nv): random values; cancellation (1e16, 1, -1e16 in scrambled lanes); one inf; inf and -inf; one NaN;
    denormals."""
    rng = _rng(18, lanes, nv)
    x = rng.normal(size=(count, lanes, nv)) * 10.0 ** rng.uniform(-8, 8, size=(count, lanes, nv))
    for i in range(count):
        kind = i % 6
        j = rng.integers(0, nv)
        l = rng.permutation(lanes)
        if kind == 1:
            x[i, :, j] = 1.0
            x[i, l[0], j], x[i, l[1], j] = 1e16, -1e16
        elif kind == 2:
            x[i, l[0], j] = np.inf
        elif kind == 3:
            x[i, l[0], j], x[i, l[1], j] = np.inf, -np.inf
        elif kind == 4:
            x[i, l[0], j] = np.nan
        elif kind == 5:
            x[i, :, j] = 5e-324 * rng.integers(1, 100, size=lanes)
    return x


def same_bits(a, b):
    """Equal bit for bit, any NaN taken as equal to any NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------------------------------------ Gram and Schur

GRAM_ROWS = (1, 63, 64, 65, 129)


def gram_cases():
    """-> rows (R, 2, 13), front (R,), counts, starts: instances of 1, 63, 64, 65 and 129 rows, each twice: every row in front,
    and one row behind the camera (its lines hold large values, which must not enter)."""
    rng = _rng(19)
    rows, front, counts, starts = [], [], [], []
    at = 0
    for n in GRAM_ROWS:
        for behind in (False, True):
            r = rng.normal(size=(n, 2, 13)) * 10.0 ** rng.uniform(-2, 2, size=(1, 1, 13))
            f = np.ones(n, np.int32)
            if behind:
                j = n // 2
                f[j] = 0
                r[j] = 1e30
            rows.append(r)
            front.append(f)
            counts.append(n)
            starts.append(at)
            at += n
    return np.concatenate(rows), np.concatenate(front), np.array(counts, np.int32), np.array(starts, np.int32)


def gram_reference(rows, front):
    """The packed 13 x 13 Gram of the rows in front, working precision -> (91,)."""
    w = rows[front != 0].reshape(-1, 13).astype(LD)
    return pack(w.T @ w)


def schur_cases(na, count=N):
    """-> m (count, packed NC x NC), scale (count,): Grams of random [J_a | J_b | r] rows, diagonal scales 1 + 10^lg."""
    rng = _rng(20, na)
    nc = na + 7
    ms, scales = [], []
    for i in range(count):
        J = rng.normal(size=(40, nc)) * 10.0 ** rng.uniform(-1, 1, size=(1, nc))
        ms.append(pack(J.T @ J))
        scales.append(1.0 + 10.0 ** float(rng.integers(-16, 3)))
    return np.array(ms), np.array(scales)


def schur_reference(na, m, scale):
    """Block elimination in the working precision -> (sc (NS + na): W U*^-1 W^T packed, then W U*^-1 g_b; yz (6 na + 6))."""
    nc = na + 7
    M = unpack(np.asarray(m).astype(LD), nc)
    U = M[na:na + 6, na:na + 6].copy()
    U[np.diag_indices(6)] *= LD(scale)
    W, gb = M[:na, na:na + 6], M[na:na + 6, nc - 1]
    Ui = _ld_inverse(U)
    Y, z = Ui @ W.T, Ui @ gb
    S = W @ Y
    return np.r_[pack(S), W @ z], np.r_[Y.ravel(), z]


def _ld_inverse(A):
    """Gauss-Jordan with partial pivoting in the working precision, refined once."""
    n = A.shape[0]
    M = np.concatenate([A.astype(LD), np.eye(n, dtype=LD)], 1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        M[[c, p]] = M[[p, c]]
        M[c] = M[c] / M[c, c]
        for r in range(n):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    X = M[:, n:]
    return X + X @ (np.eye(n, dtype=LD) - A @ X)


def schur_refusals(na):
    """m whose U block is not positive definite: a zero pivot, a negative one, a NaN."""
    m, scale = schur_cases(na, 6)
    nc = na + 7
    idx = lambda i, j: i * nc - i * (i - 1) // 2 + (j - i)
    m[0, idx(na, na)] = 0.0
    m[1, idx(na, na)] = -1.0
    m[2, idx(na + 3, na + 3)] = -1.0
    m[3, idx(na + 5, na + 5)] = -1e6
    m[4, idx(na + 1, na + 2)] = np.nan
    scale[5] = 0.0
    return m, scale


# ------------------------------------------------------------------------------------------------ frames

FRAME_ROWS = (4, 5, 63, 64, 65, 129)
FRAME_VIEWS = ("fronto", "tilt", "pi")
BOARD = cx.BOARDS[3]                         # 24 x 17: 368 ids


def pinhole_frames():
    """Noise-free frames of camera_exact.grid() on the big board: 4, 5, 63, 64, 65 and 129 rows; fronto-parallel, tilted and
    half-turn views; without distortion and with 8 coefficients -> list of grid frames."""
    return [f for f in cx.grid() if f.board == BOARD and f.sigma == 0.0 and f.view in FRAME_VIEWS and f.model in ("none", "8")]


FISH_BOARD = (24, 17, 0.012)


@functools.lru_cache(maxsize=None)
def fisheye_frames():
    """Views of a 24 x 17 board through the exact fisheye model (fisheye_exact.make_views), 4 .. 129 rows -> (objs, imgs, ids,
    poses)."""
    return fe.make_views(4100, len(FRAME_ROWS), K_FISH, fe.K_LENS, board=FISH_BOARD, rows=list(FRAME_ROWS))


def _mp_dlt(obj_xy, mn):
    """The planar DLT as the header defines it (centroids, Hartley scales, the eigenvector of the smallest eigenvalue of the
    normal matrix, denormalised, h33 = 1) in mpmath; mn = normalised image points (mpf pairs) -> H (9 floats), |H|."""
    n = len(obj_xy)
    o = [[mpf(p[0]), mpf(p[1])] for p in obj_xy]
    mc = [sum(p[c] for p in o) / n for c in range(2)]
    ic = [sum(p[c] for p in mn) / n for c in range(2)]
    a = [[p[0] - mc[0], p[1] - mc[1]] for p in o]
    b = [[p[0] - ic[0], p[1] - ic[1]] for p in mn]
    s1 = mpmath.sqrt(2) / (sum(mpmath.sqrt(p[0] ** 2 + p[1] ** 2) for p in a) / n)
    s2 = mpmath.sqrt(2) / (sum(mpmath.sqrt(p[0] ** 2 + p[1] ** 2) for p in b) / n)
    M = mpmath.zeros(9, 9)
    for (X, Y), (u, v) in zip(a, b):
        X, Y, u, v = X * s1, Y * s1, u * s2, v * s2
        for row in ([X, Y, 1, 0, 0, 0, -u * X, -u * Y, -u], [0, 0, 0, X, Y, 1, -v * X, -v * Y, -v]):
            nz = [(i, t) for i, t in enumerate(row) if t != 0]
            for i, ti in nz:
                for j, tj in nz:
                    M[i, j] += ti * tj
    E, Q = mpmath.eigsy(M)
    kmin = min(range(9), key=lambda i: E[i])
    h = [Q[i, kmin] for i in range(9)]
    H = [[h[3 * i] * s1, h[3 * i + 1] * s1, h[3 * i + 2]] for i in range(3)]
    for j in range(3):
        H[0][j] = H[0][j] / s2 + ic[0] * H[2][j]
        H[1][j] = H[1][j] / s2 + ic[1] * H[2][j]
    Hn = [H[i][j] / H[2][2] for i in range(3) for j in range(3)]
    gapw = sorted(E)[1] / max(abs(e) for e in E)
    return [float(v) for v in Hn], [float(mc[0]), float(mc[1])], float(gapw)


def pinhole_normalised_mp(cam, pix):
    """Float pixels -> the header's undistorted normalised points (five steps), mpf pairs."""
    return [list(_undistort_steps(cam, *p)[:2]) for p in pix]


def fisheye_normalised_mp(cam, pix):
    c = [mpf(t) for t in cam]
    out = []
    for p in pix:
        xp, yp = (mpf(p[0]) - c[2]) / c[0], (mpf(p[1]) - c[3]) / c[1]
        td = mpmath.sqrt(xp * xp + yp * yp)
        th = _theta_of(td, c[4:]) if td != 0 else mpmath.mpf(0)
        s = mpmath.tan(th) / td if td != 0 else mpmath.mpf(1)
        out.append([xp * s, yp * s])
    return out


def homography_gap(H, mc, ref):
    """|H - H_ref| / |H_ref| and the centroid's relative gap, max norms."""
    Hr, mr, _ = ref
    H, Hr = np.asarray(H).astype(LD), np.asarray(Hr).astype(LD)
    if not np.isfinite(np.asarray(H, np.float64)).all():
        return math.inf
    g = float(np.abs(H - Hr).max() / np.abs(Hr).max())
    return max(g, float(np.abs(np.asarray(mc) - np.asarray(mr)).max() / np.abs(mr).max()))


def pose_reference(ref):
    """The planar pose of a reference homography in the working precision: columns normalised as the header states, the polar
    factor by Newton's iteration Q <- (Q + Q^-T) / 2 -> (Q (3, 3), t)."""
    Hr, mc, _ = ref
    H = np.asarray(Hr, np.float64).reshape(3, 3).astype(LD)
    n1, n2 = np.sqrt(H[:, 0] @ H[:, 0]), np.sqrt(H[:, 1] @ H[:, 1])
    h1, h2 = H[:, 0] / n1, H[:, 1] / n2
    t = H[:, 2] * (2 / (n1 + n2))
    Q = np.stack([h1, h2, np.cross(h1, h2)], 1)
    for _ in range(30):
        Q = (Q + _ld_inverse(Q).T) / 2
    t = t - Q[:, :2] @ np.asarray(mc).astype(LD)
    return Q, t


def pose_gap(p, Qt):
    """max(|R(rvec) - Q|, |tvec - t| / |t|)."""
    Q, t = Qt
    if not np.isfinite(np.asarray(p, np.float64)).all():
        return math.inf
    g = float(np.abs(_ld_rotation(p[:3]) - Q).max())
    return max(g, float(np.abs(np.asarray(p[3:6]).astype(LD) - t).max() / np.abs(t).max()))


def normal_equations_gap(acc, ref):
    """acc = cost, JtJ (21 packed), Jtr (6) against ref = (cost, JtJ (6, 6), Jtr) -> the largest of the three relative gaps (JtJ
    by |JtJ| of its diagonal's geometric scale: entry (a, b) over sqrt(JtJ_aa JtJ_bb))."""
    cost, JtJ, Jtr = ref
    acc = np.asarray(acc).astype(LD)
    if not np.isfinite(np.asarray(acc, np.float64)).all():
        return math.inf
    d = np.sqrt(np.diag(JtJ))
    g = abs(acc[0] - cost) / cost
    g = max(g, float((np.abs(unpack(acc[1:22], 6) - JtJ) / np.outer(d, d)).max()))
    return float(max(g, float((np.abs(acc[22:28] - Jtr) / (d * np.sqrt(cost))).max())))


def pinhole_normal_equations(f, p):
    """The exact sums at pose p: camera_exact.residuals and jacobian_fd (its step 1e-6: the reference's own error is ~1e-12
    of a column, which the host statement's gap then shows and the gate inherits)."""
    obj, img, _ = cx.pool_rows(f)
    img32 = img.astype(np.float32).astype(np.float64)
    r = cx.residuals(obj, img32, p, K_PIN, cx.MODELS[f.model]).ravel()
    J = cx.jacobian_fd(obj, img32, p, K_PIN, cx.MODELS[f.model]).astype(LD)
    return r @ r, J.T @ J, J.T @ r


def fisheye_normal_equations(obj, img, p, k):
    r = (fe.project(obj, p, K_FISH, k) - cx._w(img.astype(np.float64))).ravel()
    J = fe.jacobian_fd(obj, p, K_FISH, k)[:, 8:].astype(LD)
    return r @ r, J.T @ J, J.T @ r


def pose_with_one_row_behind(obj):
    """A pose that leaves exactly one board point of obj (n, 3) at z <= 0: tilted 80 degrees, the plane z = 0 between the two
    points nearest the camera."""
    r = np.array([0.3713, 0.9285, 0.0]) * np.deg2rad(80.0)              # (an axis off the grid's directions: no two rows tie)
    R = cx.f64(cx.rotation(r))
    z = np.sort((obj.astype(np.float64) @ R.T)[:, 2])
    assert z[1] - z[0] > 1e-5
    return np.r_[r, 0.0, 0.0, -(z[0] + z[1]) / 2]


FrameSet = namedtuple("FrameSet", "name model camera board kps poses zones refs extras")


def _frame_refs(obj, mn, p, normal_equations):
    ref = _mp_dlt(obj[:, :2].astype(np.float64), mn)
    return {"H": ref, "pose": pose_reference(ref), "ne": normal_equations}


def _eval_pose(rng, r, t):
    """A pose next to the truth (1e-3 rad, 1e-3 of the depth off): residuals of a few tenths of a pixel."""
    return np.r_[r + rng.normal(size=3) * 1e-3, t + rng.normal(size=3) * 1e-3 * t[2]]


@functools.lru_cache(maxsize=None)
def pinhole_frame_set(model):
    """The frames of pinhole_frames() under one distortion model as one pool: per frame the [x, y, id] rows (id-sorted, as a pool
    holds them), the pose evaluate() is asked at, the references, and its zone (the view class).  Then the extras, whose
    verdicts are set by definition: 'behind' (a copy of the 129-row tilted frame at a pose that leaves one row at z <= 0:
    cost +inf), 'collinear ids' (DEGENERATE by the first test), 'coincident image' (by the second: three null directions) and
    'bad id' (not run)."""
    cam = cam12(K_PIN, cx.MODELS[model])
    kps, poses, zones, refs = [], [], [], []
    rng = _rng(21)
    with mpmath.workdps(DPS):
        for f in pinhole_frames():
            if f.model != model:
                continue
            obj, img, kp = cx.pool_rows(f)
            img = img.astype(np.float32).astype(np.float64)
            p = _eval_pose(rng, f.r, f.t)
            kps.append(kp)
            poses.append(p)
            zones.append(f.view)
            refs.append(dict(_frame_refs(obj, pinhole_normalised_mp(cam, img), p, pinhole_normal_equations(f, p)), truth=np.r_[f.r, f.t],
                             obj=obj.astype(np.float64), img=img))
    big = max(range(len(kps)), key=lambda i: (len(kps[i]), zones[i] == "tilt"))
    extras = {}
    obj_big = cx.board_points(kps[big][:, 2], *BOARD)
    extras["behind"] = len(kps)
    kps.append(kps[big].copy())
    poses.append(pose_with_one_row_behind(obj_big))
    line = kps[big][:7].copy()
    line[:, 2] = np.arange(7) * (BOARD[1] - 1) + 3                      # one grid row: x fixed, y = 0 .. 6
    extras["collinear ids"] = len(kps)
    kps.append(line)
    poses.append(poses[big])
    flat = kps[big][::14][:9].copy()                                  # (ids spread over the board: not collinear)
    flat[:, :2] = [120.0, 100.0]                                       # every image point the same: h31, h32, h33 are all free
    extras["coincident image"] = len(kps)
    kps.append(flat)
    poses.append(poses[big])
    bad = kps[big][:6].copy()
    bad[2, 2] = n_ids_of(BOARD)                                        # one past the board
    extras["bad id"] = len(kps)
    kps.append(bad)
    poses.append(poses[big])
    return FrameSet(f"pinhole dist {model}", "pinhole", cam, BOARD, kps, np.array(poses), zones, refs, extras)


def n_ids_of(board):
    return (board[0] - 1) * (board[1] - 1)


@functools.lru_cache(maxsize=None)
def fisheye_frame_set():
    objs, imgs, ids_l, true = fisheye_frames()
    cam = cam8(K_FISH, fe.K_LENS)
    rng = _rng(22)
    kps, poses, zones, refs = [], [], [], []
    with mpmath.workdps(DPS):
        for obj, img, ids, p_true in zip(objs, imgs, ids_l, true):
            img = img.astype(np.float64)
            p = _eval_pose(rng, p_true[:3], p_true[3:])
            kps.append(np.c_[img, ids])                                 # (make_views sorts the ids)
            poses.append(p)
            zones.append("tilt")
            refs.append(dict(_frame_refs(obj, fisheye_normalised_mp(cam, img), p, fisheye_normal_equations(obj, img, p, fe.K_LENS)),
                             truth=p_true, obj=obj.astype(np.float64), img=img))
    extras = {}
    out = kps[-1].copy()
    out[0, :2] = [cam[2] + cam[0] * 2.0, cam[3]]                        # theta_d = 2: beyond pi / 2 on this lens
    extras["outside"] = len(kps)
    kps.append(out)
    poses.append(poses[-1])
    return FrameSet("fisheye K_LENS", "fisheye", cam, FISH_BOARD, kps, np.array(poses), zones, refs, extras)
