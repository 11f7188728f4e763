"""The CPU half of the device building blocks' tests: the harness cross-compiles with the library's flags, every zone of
tests/dev_blocks_cases.py holds what it claims, the references are pinned by independent statements, and the host definition of
each block (deepcharuco_amd/pnp.py, fisheye.py; plain numpy fp64 of the same formula where there is none) is measured against the
reference zone by zone.  That table is printed here; tests/test_gpu_dev_blocks.py measures it again in its own run and gates the
device against it (dev_blocks_cases.gate).

The harness pins the source text of the blocks; the instructions inside the library's kernels stay pinned by the solver tests."""
import math
import os
import re

import mpmath
import numpy as np

import camera_exact as cx
import dev_blocks as DB
import dev_blocks_cases as Z
import fisheye_exact as fe
from deepcharuco_amd import _lm, fisheye, pnp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "deepcharuco_amd", "csrc")

# What a host statement may be off by before this file calls it wrong.  Outside the arms that are approximations by definition the
# worst dips of the fp64 statements are rvec_of's round trip next to its switch (1.5e-11), right_jacobian's cancellation just
# above its switch (4.4e-13) and the 1e-12 of camera_exact.jacobian_fd's own step; a slip in a formula is an error of 1e-3 to 1.
HOST_CEILING = 1e-9


# ------------------------------------------------------------------------------------------------ the host statements

def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])


def h_rodrigues(x):
    return np.array([pnp._rodrigues(r).ravel() for r in x])


def h_rvec_of(x):
    return np.array([pnp._rvec_of(m.reshape(3, 3)) for m in x])


def h_right_jacobian(x):
    return np.array([pnp._right_jacobian(r).ravel() for r in x])


def h_pose_basis(x):
    out = []
    for r in x:
        R, Jr = pnp._rodrigues(r), pnp._right_jacobian(r)
        out.append(np.r_[R.ravel(), (-R @ _skew([1.0, 0, 0]) @ Jr).ravel(), (-R @ _skew([0, 1.0, 0]) @ Jr).ravel()])
    return np.array(out)


def h_pose_columns(x):
    out = np.zeros((len(x), 12))
    for j in range(3):
        dX = [x[:, 6] * x[:, 8 + c * 3 + j] + x[:, 7] * x[:, 17 + c * 3 + j] for c in range(3)]
        out[:, j] = x[:, 0] * dX[0] + x[:, 1] * dX[1] + x[:, 2] * dX[2]
        out[:, 6 + j] = x[:, 3] * dX[0] + x[:, 4] * dX[1] + x[:, 5] * dX[2]
        out[:, 3 + j], out[:, 9 + j] = x[:, j], x[:, 3 + j]
    return out


def _K(cam):
    return np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1.0]])


def h_project(x):
    """pnp._project at the zero pose with the camera-frame point as its board point: residuals and d(u, v)/dq; the normalised
    and the distorted point by the same lines in plain fp64."""
    out = []
    for row in x:
        K, k, q, uv = _K(row), row[4:12], row[12:15], row[15:17]
        res, _, J = pnp._project(q[None], uv[None], np.zeros(6), K, k, True)
        iz = 1.0 / q[2]
        xx, yy = q[0] * iz, q[1] * iz
        r2 = xx * xx + yy * yy
        g = (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]))) / (1 + r2 * (k[5] + r2 * (k[6] + r2 * k[7])))
        xd = xx * g + 2 * k[2] * xx * yy + k[3] * (r2 + 2 * xx * xx)
        yd = yy * g + k[2] * (r2 + 2 * yy * yy) + 2 * k[3] * xx * yy
        out.append(np.r_[res[0], J[0, 3:], J[1, 3:], xx, yy, xd, yd])
    return np.array(out)


def h_undistort(x):
    return np.array([pnp._undistort(row[None, 12:14], _K(row), row[4:12])[0] for row in x])


def h_fisheye_distort(x):
    with np.errstate(all="ignore"):
        return np.stack(fisheye._distort(x[:, 4], x[:, 5], x[0, :4], True), 1)


def h_fisheye_project(x):
    cam = x[0]
    K, k, q, uv = _K(cam), cam[4:8], x[:, 8:11], x[:, 11:13]
    res, D = fisheye._project_q(q, uv, K, k, True)
    iz = 1.0 / q[:, 2]
    a, b = q[:, 0] * iz, q[:, 1] * iz
    d = fisheye._distort(a, b, k, False)
    return np.c_[res, D[:, 0], D[:, 1], a, b, d[0], d[1], d[2], d[3]]


def h_fisheye_undistort(x):
    cam = x[0]
    return fisheye._undistort(x[:, 8:10], _K(cam), cam[4:8])


def h_jacobi(As):
    ws, Vs = zip(*[pnp._jacobi(A) for A in As])
    return np.array(ws), np.array(Vs)


def h_polar_factor(x):
    out = []
    for m in x:
        M = m.reshape(3, 3)
        ws, W = pnp._jacobi(M.T @ M)
        out.append((M @ (W @ np.diag(1.0 / np.sqrt(ws)) @ W.T)).ravel() if ws.min() > 0 else np.full(9, np.nan))
    return np.array(out)


def h_cholesky_solve(x):
    out = []
    for row in x:
        A = Z.unpack(row[:21], 6)
        A[np.diag_indices(6)] *= row[27]
        s = _lm._cholesky_solve(A, row[21:27])
        out.append(np.full(6, np.nan) if s is None else s)
    return np.array(out)


def h_homography4(x):
    out = []
    for row in x:
        st, H, mc = pnp._homography4(np.c_[row[0:4], row[4:8]], np.c_[row[8:12], row[12:16]])
        assert st == pnp.PNP_OK
        out.append(np.r_[H.ravel(), mc])
    return np.array(out)


def h_adjugate(x):
    return np.array([pnp._adjugate(m.reshape(3, 3)).ravel() for m in x])


def h_projective_basis(x):
    return np.array([pnp._projective_basis(np.c_[row[:4], row[4:]]).ravel() for row in x])


# block -> (zones, host statement): the per-lane continuous blocks with a plain (out) interface
def lane_blocks():
    za, zp = Z.adjugate_zones()
    return {
        "rodrigues": (Z.rodrigues_zones(), h_rodrigues), "rvec_of": (Z.rvec_of_zones(), h_rvec_of),
        "right_jacobian": (Z.right_jacobian_zones(), h_right_jacobian), "pose_basis": (Z.pose_basis_zones(), h_pose_basis),
        "pose_columns": (Z.pose_columns_zones(), h_pose_columns), "project": (Z.project_zones(), h_project),
        "undistort": (Z.undistort_zones(), h_undistort), "fisheye_distort": (Z.fisheye_distort_zones(), h_fisheye_distort),
        "fisheye_project": (Z.fisheye_project_zones(), h_fisheye_project),
        "fisheye_undistort": (Z.fisheye_undistort_zones(), h_fisheye_undistort),
        "polar_factor": (Z.polar_factor_zones(), h_polar_factor), "cholesky_solve": (Z.cholesky_zones(), h_cholesky_solve),
        "homography4": (Z.homography4_zones(), h_homography4), "adjugate": ([za], h_adjugate),
        "projective_basis": ([zp], h_projective_basis),
    }


def ceiling(block, zone):
    if block == "cholesky_solve":
        return max(HOST_CEILING, 64 * Z.EPS * float(zone.name.split()[1]))        # the solve's own conditioning: eps * cond
    return HOST_CEILING


def host_table():
    """-> {(block, zone name): g_host}, in the blocks' order."""
    table = {}
    for block, (zones, host) in lane_blocks().items():
        for z in zones:
            table[block, z.name] = z.measure(host(z.x))
    return table


def host_jacobi_table(n, count):
    out = {}
    for name, (As, w_ref) in Z.eigen_reference(n, count).items():
        ws, Vs = h_jacobi(As)
        out[name] = Z.jacobi_gap(As, w_ref, ws, Vs)
    return out


def print_table(title, table):
    print(f"\n{title}")
    for key, g in table.items():
        name = " / ".join(key) if isinstance(key, tuple) else key
        print(f"  {name:<58s} " + (" ".join(f"{v:9.2e}" for v in g) if isinstance(g, tuple) else f"{g:9.2e}"))


# ------------------------------------------------------------------------------------------------ the harness builds

def _make_vars(path):
    text = open(path).read()
    return {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}, text


def test_harness_uses_the_librarys_flags():
    mine, mine_text = _make_vars(os.path.join(REPO, "tests", "csrc", "Makefile"))
    lib, lib_text = _make_vars(os.path.join(CSRC, "Makefile"))
    for var in ("HIPCC", "ARCH", "CXXFLAGS"):
        assert mine[var] == lib[var], var
    assert "--offload-arch=$(ARCH)" in mine["CXXFLAGS"] and lib["ARCH"] == "gfx950"
    compile_line = lambda t: re.search(r"^\t(\$\(HIPCC\) \$\(CXXFLAGS\).*) -c ", t, re.M).group(1)
    link_line = lambda t: re.search(r"^\t(\$\(HIPCC\) -shared \S+ \S+) ", t, re.M).group(1)
    assert compile_line(mine_text) == compile_line(lib_text)
    assert link_line(mine_text) == link_line(lib_text)


def test_harness_cross_compiles_and_refuses_bad_arguments():
    path = DB.build()
    assert os.path.exists(path) and not DB.stale()
    with open(path, "rb") as f:
        assert b"gfx950" in f.read()
    h = DB.lib()
    cap = h.dcxt_cap()
    assert cap == 65536
    one = np.zeros(4096)
    p = one.ctypes.data                      # a host address: never dereferenced, every call below is refused before it launches
    for name in DB.BLOCKS:
        fn = getattr(h, "dcxt_" + name)
        for args in ((None, p, p, p, 1), (p, None, p, p, 1), (p, p, None, p, 1), (p, p, p, None, 1), (p, p, p, p, 0), (p, p, p, p, -1),
                     (p, p, p, p, cap + 1)):
            assert fn(*args, None) == -1, (name, args)
    assert h.dcxt_ransac_sample(None, 4, p, p, 1, None) == -1 and h.dcxt_ransac_sample(p, 0, p, p, 1, None) == -1
    assert h.dcxt_ransac_sample(p, 4, p, p, cap + 1, None) == -1 and h.dcxt_ransac_sample(p, 4, p, None, 1, None) == -1
    assert h.dcxt_best_hypothesis(None, 4, p, p, 1, None) == -1 and h.dcxt_best_hypothesis(p, 0, p, p, 1, None) == -1
    assert h.dcxt_best_hypothesis(p, 4, p, p, 0, None) == -1 and h.dcxt_best_hypothesis(p, 4, p, p, cap + 1, None) == -1
    for fn in (h.dcxt_block_tree6, h.dcxt_block_tree7):
        assert fn(None, p, 1, None) == -1 and fn(p, None, 1, None) == -1 and fn(p, p, 0, None) == -1 and fn(p, p, cap + 1, None) == -1
    assert h.dcxt_accumulate_rows(None, p, 1, p, p, p, p, 1, None) == -1 and h.dcxt_accumulate_rows(p, p, 0, p, p, p, p, 1, None) == -1
    assert h.dcxt_accumulate_rows(p, p, 1, p, p, p, p, cap + 1, None) == -1
    for na in (6, 8, 9):
        fn = getattr(h, f"dcxt_schur_view{na}")
        assert fn(None, p, p, p, p, 1, None) == -1 and fn(p, p, p, p, p, 0, None) == -1 and fn(p, p, p, p, p, cap + 1, None) == -1
    pool_ok = (p, p, p, p, 1, 8, 24, 17, 0.004)
    assert h.dcxt_frame_checks(*pool_ok, None, None) == -1
    assert h.dcxt_frame_checks(None, p, p, p, 1, 8, 24, 17, 0.004, p, None) == -1
    assert h.dcxt_frame_checks(p, p, p, p, 0, 8, 24, 17, 0.004, p, None) == -1
    assert h.dcxt_frame_checks(p, p, p, p, cap + 1, 8, 24, 17, 0.004, p, None) == -1
    assert h.dcxt_frame_checks(p, p, p, p, 1, -1, 24, 17, 0.004, p, None) == -1
    for fn in (h.dcxt_frame_blocks_pinhole, h.dcxt_frame_blocks_fisheye):
        assert fn(*pool_ok, None, p, p, p, None) == -1 and fn(*pool_ok, p, p, p, None, None) == -1
        assert fn(p, p, p, p, cap + 1, 8, 24, 17, 0.004, p, p, p, p, None) == -1
        assert fn(p, p, None, p, 1, 8, 24, 17, 0.004, p, p, p, p, None) == -1


def test_thresholds_named_by_the_zones_are_the_headers():
    cam = open(os.path.join(CSRC, "dcx_camera_dev.h")).read()
    fish = open(os.path.join(CSRC, "dcx_fisheye_dev.h")).read()
    assert float(re.search(r"if \(!\(th >= ([0-9.e+-]+)\)\)", cam).group(1)) == Z.TH_IDENTITY
    assert float(re.search(r"if \(s < ([0-9.e+-]+)\)", cam).group(1)) == Z.S_SMALL
    assert float(re.search(r"if \(th2 < ([0-9.e+-]+)\)", cam).group(1)) == Z.TH2_SERIES
    assert re.search(r"kFisheyeSmallR = 1e-4;", fish) and Z.SMALL_R == 1e-4
    assert re.search(r"kFisheyeSmallThetaD = 1e-8;", fish) and Z.SMALL_THETA_D == 1e-8
    assert "kUndistortIters = 5;" in cam


# ------------------------------------------------------------------------------------------------ the zones

def test_every_zone_holds_what_it_claims():
    seen = {}
    for block, (zones, _) in lane_blocks().items():
        for z in zones:
            assert len(z.x) >= 64, (block, z.name, len(z.x))
            Z.check_sides(z)
            for label, _, switch, side in z.sides:
                seen.setdefault((block, label, switch), set()).add(side)
    # both sides of every switch that a block's text has
    for key in (("rodrigues", "th", Z.TH_IDENTITY), ("rvec_of", "s", Z.S_SMALL), ("right_jacobian", "th2", Z.TH2_SERIES),
                ("pose_basis", "th2", Z.TH2_SERIES), ("fisheye_distort", "r", Z.SMALL_R),
                ("fisheye_undistort", "theta_d", Z.SMALL_THETA_D)):
        assert seen[key] == {"<", ">"}, key
    names = [z.name for z in Z.undistort_zones()]
    assert "dist neg / icdist < 0" in names and "dist none / field" in names
    verdicts = {int(v) for z in Z.fisheye_undistort_zones() for v in z.expect}
    assert verdicts == {0, 1}
    # rvec_of's half-turn arm: every sign pattern of the axis, axes with a zero component, and the x-smallest fix-up
    M = dict(Z.rvec_matrices())["s < 1e-5, c < 0"][0]
    ref = np.array([cx.f64(Z._rvec_definition_ld(m)) for m in M])
    patterns = {tuple(int(np.sign(v)) if abs(v) > 1e-4 else 0 for v in r) for r in ref}       # (pi - th < 1e-5 leaves ~1e-5 there)
    assert len({p for p in patterns if 0 not in p}) >= 4 and any(0 in p for p in patterns)
    x, y, z_ = np.abs(ref).T
    fix = (x < y) & (x < z_)
    assert fix.sum() >= 8
    q = Z.behind_points()
    assert not (q[:, 2] > 0).any()


def test_reduction_restatements():
    x = Z.reduction_inputs(64, 5, 12)
    for a in x:
        s = Z.butterfly(a)
        assert Z.same_bits(s, np.tile(s[0], (64, 1)))           # fp64 addition commutes: the butterfly leaves one value in all lanes
    a = np.arange(64.0 * 5).reshape(64, 5)                              # small integers: every order gives the exact sum
    assert np.array_equal(Z.butterfly(a), np.tile(a.sum(0), (64, 1)))
    t = Z.tree(np.arange(1024.0 * 6).reshape(1024, 6))
    assert np.array_equal(t, np.arange(1024.0 * 6).reshape(1024, 6).sum(0))


# ------------------------------------------------------------------------------------------------ the references are pinned

def test_references_are_pinned():
    rng = np.random.default_rng(5)
    with mpmath.workdps(40):
        # the rotation: closed form against mpmath.expm and against camera_exact.rotation
        for r in [np.zeros(3), np.array([1e-300, 0, 0]), rng.normal(size=3) * 1e-9, rng.normal(size=3), np.array([0.0, 0, np.pi]),
                  rng.normal(size=3) * 3.0]:
            R = Z.mp_rotation([Z.mpf(v) for v in r])
            E = mpmath.expm(mpmath.matrix([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]))
            L = cx.rotation(r)
            for i in range(3):
                for j in range(3):
                    assert abs(R[i][j] - E[i, j]) < mpmath.mpf(10) ** -35
                    assert abs(R[i][j] - cx.to_mp(L[i, j])) < 3e-19
        # the two camera models against the 64-bit-mantissa statements
        for dist in cx.MODELS.values():
            xy = rng.uniform(-0.5, 0.5, size=(4, 2))
            L = cx.distort(cx._w(xy[:, 0]), cx._w(xy[:, 1]), np.eye(3), cx.dist8(dist))
            for i in range(4):
                m = Z.mp_pinhole(Z.mpf(xy[i, 0]), Z.mpf(xy[i, 1]), [Z.mpf(v) for v in cx.dist8(dist)])
                assert abs(m[0] - cx.to_mp(L[i, 0])) < 3e-19 and abs(m[1] - cx.to_mp(L[i, 1])) < 3e-19
        for k in Z.FISH_LENSES.values():
            ab = np.r_[np.zeros((1, 2)), [[1e-12, 0]], rng.uniform(-2, 2, size=(4, 2)), [[300.0, 400.0]]]
            L = fe.distort(ab[:, 0], ab[:, 1], np.eye(3), k)
            for i in range(len(ab)):
                m = Z.mp_fisheye(Z.mpf(ab[i, 0]), Z.mpf(ab[i, 1]), [Z.mpf(v) for v in k])
                assert abs(m[0] - cx.to_mp(L[i, 0])) < 5e-19 and abs(m[1] - cx.to_mp(L[i, 1])) < 5e-19
    # the derivative recipe against camera_exact.jacobian_fd's (its own step: 1e-6, error ~1e-12): Jr through d(R m)/dr
    with mpmath.workdps(Z.DPS):
        r = np.array([0.3, -0.2, 0.5])
        Jr = np.array(Z._jr_and_g(r)[0]).reshape(3, 3)
    h = 1e-6
    R0 = cx.rotation(r)
    for j in range(3):
        d = np.zeros(3)
        d[j] = h
        dR = (cx.rotation(r + d) - cx.rotation(r - d)) / (2 * cx.LD(h))
        Wm = cx.f64(R0.T @ dR)
        assert np.abs(np.array([Wm[2, 1], Wm[0, 2], Wm[1, 0]]) - Jr[:, j]).max() < 1e-10
    # the five-step inverse against camera_exact.undistort5 (no icdist < 0 on these lenses)
    with mpmath.workdps(Z.DPS):
        for dist in (cx.MODELS["5"], cx.MODELS["8"]):
            pix = rng.uniform(60, 260, size=(4, 2))
            L = cx.undistort5(pix, Z.K_PIN, dist)
            for i in range(4):
                x, y, _ = Z._undistort_steps(Z.cam12(Z.K_PIN, dist), *pix[i])
                assert abs(x - cx.to_mp(L[i, 0])) < 1e-17 and abs(y - cx.to_mp(L[i, 1])) < 1e-17
    # the fisheye root: theta_d of the root is theta_d
    with mpmath.workdps(Z.DPS):
        k = [Z.mpf(v) for v in fe.K_LENS]
        for td in (1e-8, 0.3, 1.2):
            th = Z._theta_of(Z.mpf(td), k)
            assert abs(th * (1 + k[0] * th ** 2 + k[1] * th ** 4 + k[2] * th ** 6 + k[3] * th ** 8) - Z.mpf(td)) < mpmath.mpf(10) ** -35
    # the polar factor and the four-point homography by their defining properties
    with mpmath.workdps(Z.DPS):
        M = rng.normal(size=9)
        Q = np.array(Z._mp_polar(M)).reshape(3, 3)
        assert np.abs(Q.T @ Q - np.eye(3)).max() < 1e-15
        P = Q.T @ M.reshape(3, 3)
        assert np.abs(P - P.T).max() < 1e-14 and np.linalg.eigvalsh((P + P.T) / 2).min() > 0
        objs, imgs = Z.quadruples()["general"]
        H, mc = Z._mp_homography4(objs[0], imgs[0])
        w = np.c_[objs[0] - mc, np.ones(4)] @ np.array(H).reshape(3, 3).T
        assert np.abs(w[:, :2] / w[:, 2:] - imgs[0]).max() < 1e-13
    # the DLT reference: through four points it is the eight-equation solve's homography (two statements, one answer)
    fs = Z.pinhole_frame_set("none")
    four = [i for i, kp in enumerate(fs.kps[:len(fs.refs)]) if len(kp) == 4]
    assert len(four) == 3
    with mpmath.workdps(Z.DPS):
        for i in four:
            ref = fs.refs[i]
            mn = [[float(v) for v in p] for p in Z.pinhole_normalised_mp(fs.camera, ref["img"])]
            H4, mc = Z._mp_homography4(ref["obj"][:, :2], mn)
            assert np.abs(np.array(H4) - ref["H"][0]).max() <= 1e-12 * np.abs(H4).max() and np.allclose(mc, ref["H"][1], rtol=1e-15)
    # the Schur reference: block elimination against the plain inverse of the whole matrix
    m, scale = Z.schur_cases(6, 2)
    sc, yz = Z.schur_reference(6, m[0], scale[0])
    Mf = Z.unpack(m[0], 13)
    U = Mf[6:12, 6:12].copy()
    U[np.diag_indices(6)] *= scale[0]
    assert np.allclose(cx.f64(sc[:21]), Z.pack(Mf[:6, 6:12] @ np.linalg.solve(U, Mf[6:12, :6])), rtol=1e-9)
    assert np.allclose(cx.f64(yz[36:]), np.linalg.solve(U, Mf[6:12, 12]), rtol=1e-9)


# ------------------------------------------------------------------------------------------------ the host table

def test_host_statements_per_zone():
    table = host_table()
    print_table("host fp64 statement against the reference, per zone (max gap over the zone, divided by the output's size)", table)
    blocks = lane_blocks()
    for (block, name), g in table.items():
        zone = next(z for z in blocks[block][0] if z.name == name)
        assert g <= ceiling(block, zone), (block, name, g)
    # the arms that are exact by definition
    for z in Z.rvec_of_zones():
        if z.expect == "exactly zero":
            assert not h_rvec_of(z.x).any()
    # undistort where five steps have converged: the true inverse, to the bound derived at dev_blocks_cases.conv_bound
    for z in Z.undistort_zones():
        if z.expect is not None:
            assert np.abs(h_undistort(z.x) - z.expect[0]).max() <= z.expect[1] + 4 * Z.EPS, z.name
    # the verdicts
    for z in Z.fisheye_undistort_zones():
        assert np.array_equal(~np.isnan(h_fisheye_undistort(z.x)).any(1), z.expect.astype(bool)), z.name
    assert np.isnan(h_polar_factor(Z.singular_matrices())).all()
    assert np.isnan(h_cholesky_solve(Z.cholesky_refusals())).all()


def test_host_jacobi_per_zone():
    for n, count in ((3, Z.JACOBI3_COUNT), (9, Z.JACOBI9_COUNT)):
        table = host_jacobi_table(n, count)
        print_table(f"pnp._jacobi {n} x {n}: |V^T V - I|, |A V - V w| / |A|, |w - eigsy| / |A|", table)
        for name, g in table.items():
            assert max(g) <= HOST_CEILING, (n, name, g)


def test_host_gram_and_schur():
    rows, front, counts, starts = Z.gram_cases()
    worst = 0.0
    for n, s in zip(counts, starts):
        r, f = rows[s:s + n], front[s:s + n]
        ref = Z.gram_reference(r, f)
        w = r[f != 0].reshape(-1, 13)
        got = Z.pack(w.T @ w)
        d = np.sqrt(np.abs(cx.f64(Z.unpack(ref, 13)).diagonal()))
        d[d == 0] = 1.0                                   # (the one-row instance whose row is behind: an empty sum)
        worst = max(worst, float((np.abs(Z.unpack(got - ref, 13)) / np.outer(d, d).astype(cx.LD)).max()))
    print(f"\nGram of [J | r] rows, numpy fp64 against the working precision: {worst:.2e}")
    assert worst <= HOST_CEILING
    for na in (6, 8, 9):
        g = schur_host_gap(na)
        print(f"schur_view<{na}>, numpy fp64 block elimination against the working precision: {g:.2e}")
        assert g <= HOST_CEILING


def schur_numpy(na, m, scale):
    """Plain fp64 of the header's formula: U* = U with its diagonal scaled, Y = U*^-1 W^T, z = U*^-1 g_b by Cholesky."""
    nc = na + 7
    M = Z.unpack(m, nc)
    U = M[na:na + 6, na:na + 6].copy()
    U[np.diag_indices(6)] *= scale
    W, gb = M[:na, na:na + 6], M[na:na + 6, nc - 1]
    Y = np.stack([_lm._cholesky_solve(U, W[j]) for j in range(na)], 1)
    z = _lm._cholesky_solve(U, gb)
    return np.r_[Z.pack(W @ Y), W @ z], np.r_[Y.ravel(), z]


def schur_gap(na, m, sc, yz):
    """sc and yz against the reference, each entry over the natural size of its row and column."""
    g = 0.0
    for mi, si, sci, yzi in zip(*m, sc, yz):
        rs, ry = Z.schur_reference(na, mi, si)
        g = max(g, float(np.abs(sci - rs).max() / np.abs(rs).max()), float(np.abs(yzi - ry).max() / np.abs(ry).max()))
    return g if math.isfinite(g) else math.inf


def schur_host_gap(na):
    m = Z.schur_cases(na)
    out = [schur_numpy(na, mi, si) for mi, si in zip(*m)]
    return schur_gap(na, m, [o[0] for o in out], [o[1] for o in out])


def test_pk_and_unpk_are_inverse_on_the_host_side():
    for n in DB.UNPK_N:
        e = 0
        for i in range(n):
            for j in range(i, n):
                assert i * n - i * (i - 1) // 2 + (j - i) == e
                e += 1
        assert e == n * (n + 1) // 2


# ------------------------------------------------------------------------------------------------ frames

def frame_sets():
    return [Z.pinhole_frame_set("none"), Z.pinhole_frame_set("8"), Z.fisheye_frame_set()]


def host_frame_results(fs):
    """pnp's / fisheye's statements on every reference frame of the set -> list of (H (9), mc (2), p0 (6), acc (28))."""
    K, k = _K(fs.camera), fs.camera[4:]
    out = []
    for ref, p in zip(fs.refs, fs.poses):
        obj, img = ref["obj"], ref["img"]
        und, proj = (pnp._undistort, pnp._project) if fs.model == "pinhole" else (fisheye._undistort, fisheye._project)
        mn = und(img, K, k)
        st, H, mc = pnp._homography(obj, mn)
        st2, p0 = pnp._init_pose(obj, mn)
        assert st == st2 == pnp.PNP_OK
        res, cost, J = proj(obj, img, p, K, k, True)
        out.append((H.ravel(), mc, p0, np.r_[cost, Z.pack(J.T @ J), J.T @ res.ravel()]))
    return out


def frame_gaps(fs, results):
    """-> {zone: (H gap, init pose gap, normal equations gap)}: the zone's maxima over its frames."""
    gaps = {}
    for ref, zone, (H, mc, p0, acc) in zip(fs.refs, fs.zones, results):
        g = (Z.homography_gap(H, mc, ref["H"]), Z.pose_gap(p0, ref["pose"]), Z.normal_equations_gap(acc, ref["ne"]))
        gaps[zone] = tuple(max(a, b) for a, b in zip(gaps.get(zone, (0.0, 0.0, 0.0)), g))
    return gaps


# The init pose against the truth: a sanity bound, not a rounding bound.  The image points are float32 (half an ulp at 256 px is
# 1.5e-5 px, over triangles at least 10 px high), five undistort steps leave ~1e-7 at the field's edge, and inside rvec_of's
# s < 1e-5 arms the rotation is snapped by up to 9e-6: all far below 1e-3, while a wrong sign or a transposed matrix is of size 1.
TRUTH_BOUND = 1e-3


def truth_gap(p0, truth):
    return max(cx.rot_gap(p0[:3], truth[:3]), float(np.abs(p0[3:6] - truth[3:6]).max() / np.abs(truth[3:6]).max()))


def test_host_frames_per_zone():
    for fs in frame_sets():
        res = host_frame_results(fs)
        gaps = frame_gaps(fs, res)
        print_table(f"{fs.name}: homography, init_pose, evaluate (cost, JtJ, Jtr) of the host statements against the references", gaps)
        for zone, g in gaps.items():
            assert g[0] <= HOST_CEILING and g[2] <= 1e-9, (fs.name, zone, g)
            # the init pose passes through rvec_of: inside its s < 1e-5 arms (fronto-parallel and half-turn views) the rotation is
            # an approximation by definition, off by up to 9e-6
            assert g[1] <= (1e-4 if zone in ("fronto", "pi") else HOST_CEILING), (fs.name, zone, g)
        for ref, r in zip(fs.refs, res):
            assert truth_gap(r[2], ref["truth"]) <= TRUTH_BOUND
        # the frames whose verdict is set by definition: the host definition gives it too
        if fs.model == "pinhole":
            K, k = _K(fs.camera), fs.camera[4:]
            for name in ("collinear ids", "coincident image"):
                kp = fs.kps[fs.extras[name]]
                obj = cx.board_points(kp[:, 2], *fs.board).astype(np.float64)
                assert pnp._homography(obj, pnp._undistort(kp[:, :2], K, k))[0] == pnp.PNP_DEGENERATE, name
            kp, p = fs.kps[fs.extras["behind"]], fs.poses[fs.extras["behind"]]
            obj = cx.board_points(kp[:, 2], *fs.board).astype(np.float64)
            z = (obj @ pnp._rodrigues(p[:3]).T + p[3:])[:, 2]
            assert (z <= 0).sum() == 1 and pnp._project(obj, kp[:, :2], p, K, k, False)[1] == math.inf
