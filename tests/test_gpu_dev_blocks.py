"""The fp64 device building blocks (csrc/dcx_mat_dev.h, dcx_camera_dev.h, dcx_fisheye_dev.h, dcx_pnp_dev.h) one by one on the device,
through the thin kernels of tests/csrc/dev_blocks.hip, against exact math.

The gate ("The device building blocks one by one"): for a continuous block and a zone, g_host is the zone maximum of
the fp64 host statement against the reference, measured in this run by tests/test_dev_blocks_host.py's statements; the device
passes if its zone maximum is at most 8 * max(g_host, 4 eps), both divided by the output's natural size in the zone.  Discrete
blocks and the fixed-order reductions are held by exact equality.  Every test prints the device's gap beside the host's.

The harness pins the source text of the blocks, compiled with the library's flags in a translation unit of its own.  It does not
pin the instructions inside the library's kernels; those stay pinned end to end by the solver tests."""
import numpy as np
import pytest
import torch

import camera_exact as cx
import dev_blocks as DB
import dev_blocks_cases as Z
import pool_cases
import test_dev_blocks_host as HT
from deepcharuco_amd import corner_pool, pnp
from test_gpu_pose_edges import _agree_rot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def dev():
    assert torch.cuda.is_available()
    DB.lib()
    return torch.device("cuda", 0)


def _report(block, zone, g_host, g_dev):
    bound = Z.gate(g_host)
    print(f"  {block + ' / ' + zone:<60s} host {g_host:9.2e}  device {g_dev:9.2e}  gate {bound:9.2e}{'' if g_dev <= bound else '   <-- over'}")
    return g_dev <= bound


def _gate_lane_block(block, run=None):
    """Every zone of a per-lane block: device and host gaps printed, the gate asserted after the table is whole."""
    zones, host = HT.lane_blocks()[block]
    print(f"\n{block}")
    over, outs = [], {}
    for z in zones:
        out, iout = DB.run(run or block, z.x)
        outs[z.name] = (out, iout)
        if not _report(block, z.name, z.measure(host(z.x)), z.measure(out)):
            over.append(z.name)
    assert not over, (block, over)
    return outs


# ------------------------------------------------------------------------------------------------ rotations

def test_rotations():
    _gate_lane_block("rodrigues")
    outs = _gate_lane_block("rvec_of")
    assert not outs["s < 1e-5, c > 0"][0].any()                           # exactly zero, every sign bit clear or not: zero
    _gate_lane_block("right_jacobian")
    _gate_lane_block("pose_basis")
    _gate_lane_block("pose_columns")
    # the identity arm returns the identity's bits
    out, _ = DB.run("rodrigues", Z.rotation_vectors()["1e-301"])
    assert np.array_equal(out, np.tile(np.eye(3).ravel(), (len(out), 1)))


# ------------------------------------------------------------------------------------------------ the two camera models

def _pixel_bound():
    return Z.gate(0.0) * 1000.0            # two evaluations of one formula in one format, pixels below 1000


def test_pinhole_model():
    outs = _gate_lane_block("project")
    for z in Z.project_zones():
        out = outs[z.name][0]
        assert (outs[z.name][1] == 1).all()
        nj, ok = DB.run("project_nojac", z.x)
        assert (ok == 1).all() and np.abs(nj - out[:, :2]).max() <= _pixel_bound(), z.name
        # distort() by itself on the normalised points project() reported: the same values, and a, b, d behind du, dv
        k, x, y = z.x[:, 4:12], out[:, 8], out[:, 9]
        d, _ = DB.run("distort", np.c_[k, x, y])
        scale = max(np.abs(out[:, 10:12]).max(), 1e-300)
        assert np.abs(d[:, :2] - out[:, 10:12]).max() <= Z.gate(0.0) * scale, z.name
        iz = 1.0 / z.x[:, 14]
        du0, du1, dv1 = z.x[:, 0] * d[:, 2] * iz, z.x[:, 0] * d[:, 3] * iz, z.x[:, 1] * d[:, 4] * iz
        for got, want in ((out[:, 2], du0), (out[:, 3], du1), (out[:, 6], dv1)):
            assert np.abs(got - want).max() <= Z.gate(0.0) * np.abs(want).max(), z.name
    # q_z <= 0: false, nothing written
    q = Z.behind_points()
    x = np.c_[np.tile(Z.cam12(Z.K_PIN, cx.MODELS["8"]), (len(q), 1)), q, np.zeros((len(q), 2))]
    for block in ("project", "project_nojac"):
        out, ok = DB.run(block, x)
        assert (ok == 0).all() and DB.untouched(out).all(), block
    outs = _gate_lane_block("undistort")
    for z in Z.undistort_zones():
        if z.expect is not None:                                       # five steps have converged: the true inverse
            gap = np.abs(outs[z.name][0] - z.expect[0]).max()
            print(f"  undistort / {z.name}: against the true inverse {gap:.2e} (bound {z.expect[1]:.2e})")
            assert gap <= z.expect[1] + 4 * Z.EPS, z.name


def test_fisheye_model():
    _gate_lane_block("fisheye_distort")
    outs = _gate_lane_block("fisheye_project")
    for z in Z.fisheye_project_zones():
        assert (outs[z.name][1] == 1).all()
        nj, ok = DB.run("fisheye_project_nojac", z.x)
        assert (ok == 1).all() and np.abs(nj - outs[z.name][0][:, :2]).max() <= _pixel_bound(), z.name
    q = Z.behind_points()
    x = np.c_[np.tile(Z.cam8(Z.K_FISH, Z.FISH_LENSES["K_LENS"]), (len(q), 1)), q, np.zeros((len(q), 2))]
    for block in ("fisheye_project", "fisheye_project_nojac"):
        out, ok = DB.run(block, x)
        assert (ok == 0).all() and DB.untouched(out).all(), block
    outs = _gate_lane_block("fisheye_undistort")
    for z in Z.fisheye_undistort_zones():
        out, inside = outs[z.name]
        assert np.array_equal(inside[:, 0], z.expect), z.name
        assert np.array_equal(np.isnan(out).all(1), z.expect == 0) and np.array_equal(np.isnan(out).any(1), z.expect == 0), z.name


# ------------------------------------------------------------------------------------------------ small matrices

def _jacobi_rows(block, name, host, device):
    ok = True
    for label, gh, gd in zip(("V^T V - I", "A V - V w", "w - eigsy"), host, device):
        ok &= _report(block, f"{name}: {label}", gh, gd)
    return ok


def test_jacobi_3x3():
    print("\njacobi<3, 3>")
    host = HT.host_jacobi_table(3, Z.JACOBI3_COUNT)
    over = []
    for name, (As, w_ref) in Z.eigen_reference(3, Z.JACOBI3_COUNT).items():
        out, _ = DB.run("jacobi3", np.array([Z.pack(A) for A in As]))
        ws = np.array([Z.unpack(o[:6], 3).diagonal() for o in out])
        if not _jacobi_rows("jacobi<3, 3>", name, host[name], Z.jacobi_gap(As, w_ref, ws, out[:, 6:].reshape(-1, 3, 3))):
            over.append(name)
    assert not over, over


def test_jacobi_9x9_in_every_lane():
    print("\njacobi<9, 1>: the lanes' rows assembled into V")
    host = HT.host_jacobi_table(9, Z.JACOBI9_COUNT)
    over = []
    for name, (As, w_ref) in Z.eigen_reference(9, Z.JACOBI9_COUNT).items():
        out, _ = DB.run("jacobi9", np.array([Z.pack(A) for A in As]))             # (n, 64, 54)
        M = out[:, :, :45]
        assert Z.same_bits(M, np.repeat(M[:, :1], 64, 1)), name                  # every lane rotated the same matrix
        assert not out[:, 9:, 45:].any(), name                                     # rows past the ninth stay zero
        ws = np.array([Z.unpack(m, 9).diagonal() for m in M[:, 0]])
        if not _jacobi_rows("jacobi<9, 1>", name, host[name], Z.jacobi_gap(As, w_ref, ws, out[:, :9, 45:])):
            over.append(name)
    assert not over, over


def test_polar_factor_and_cholesky():
    _gate_lane_block("polar_factor")
    for z in Z.polar_factor_zones():
        assert (DB.run("polar_factor", z.x)[1] == 1).all(), z.name
    out, ok = DB.run("polar_factor", Z.singular_matrices())
    assert (ok == 0).all() and DB.untouched(out).all()
    outs = _gate_lane_block("cholesky_solve")
    print("\ncholesky_factor<6> and cholesky_substitute<6>")
    for z in Z.cholesky_zones():
        assert (outs[z.name][1] == 1).all()
        L, ok = DB.run("cholesky_factor", np.c_[z.x[:, :21], z.x[:, 27]])
        assert (ok == 1).all()
        want = np.array([Z.lower_packed_to_pk(l) for l in z.expect])
        # L against the factor in mpmath, relative to the factor's size; the host side of this gate is _lm._cholesky_solve's
        # solution gap of the same zone (the factor's error is what the solution's is made of)
        g_dev = float((np.abs(L - want).max(1) / np.abs(want).max(1)).max())
        g_host = z.measure(HT.h_cholesky_solve(z.x))
        assert _report("cholesky_factor", z.name, g_host, g_dev)
        x, _ = DB.run("cholesky_substitute", np.c_[L, z.x[:, 21:27]])
        assert _report("cholesky_substitute", z.name, g_host, z.measure(x))
    for block, x in (("cholesky_solve", Z.cholesky_refusals()), ("cholesky_factor", Z.cholesky_refusals()[:, list(range(21)) + [27]])):
        out, ok = DB.run(block, x)
        assert (ok == 0).all() and DB.untouched(out).all(), block


def test_four_point_blocks():
    _gate_lane_block("adjugate")
    _gate_lane_block("projective_basis")
    outs = _gate_lane_block("homography4")
    print("\ninit_pose through the four-point homography")
    for z in Z.homography4_zones():
        assert (outs[z.name][1] == pnp.PNP_OK).all()
        p0, st = DB.run("init_pose4", z.x)
        assert (st == pnp.PNP_OK).all()
        refs = [Z.pose_reference((list(r[:9]), list(r[9:]), None)) for r in _mp_h4(z)]
        g_dev = max(Z.pose_gap(p, r) for p, r in zip(p0, refs))
        host = []
        for row in z.x:
            _, H, mc = pnp._homography4(np.c_[row[0:4], row[4:8]], np.c_[row[8:12], row[12:16]])
            host.append(pnp._pose_of_homography(H, mc)[1])
        g_host = max(Z.pose_gap(p, r) for p, r in zip(host, refs))
        assert _report("init_pose4", z.name, g_host, g_dev)


def _mp_h4(zone):
    import mpmath
    with mpmath.workdps(Z.DPS):
        out = []
        for row in zone.x:
            H, mc = Z._mp_homography4(np.c_[row[0:4], row[4:8]], np.c_[row[8:12], row[12:16]])
            out.append(np.r_[H, mc])
        return out


# ------------------------------------------------------------------------------------------------ reductions

def test_wave_sum_leaves_the_same_bits_in_all_64_lanes():
    for nv, block in ((5, "wave_sum5"), (28, "wave_sum28")):
        x = Z.reduction_inputs(64, nv, 24)
        out, _ = DB.run(block, x.reshape(len(x), -1))
        for a, o in zip(x, out):
            assert Z.same_bits(o, Z.butterfly(a)), block                              # bit for bit the restated butterfly
            assert Z.same_bits(o, np.repeat(o[:1], 64, 0)), block                    # and one value in all 64 lanes


def test_block_tree():
    t = DB.block_tree_threads()
    assert t == 1024
    for nv in (6, 7):
        x = Z.reduction_inputs(t, nv, 12)
        out = DB.block_tree(x)
        for a, o in zip(x, out):
            assert Z.same_bits(o, Z.tree(a)), nv


# ------------------------------------------------------------------------------------------------ discrete blocks

def test_append_kept():
    rng = np.random.default_rng(31)
    masks = [np.zeros(64, int), np.ones(64, int), np.arange(64) % 2, (np.arange(64) + 1) % 2]
    masks += [(np.arange(64) == l).astype(int) for l in (0, 1, 31, 32, 63)] + [rng.integers(0, 2, size=64) for _ in range(8)]
    counts = rng.integers(0, 1000, size=len(masks))
    counts[:4] = [0, 7, 0, 2 ** 31 - 1 - 64]
    _, io = DB.run("append_kept", ix=np.c_[np.array(masks), counts])
    for m, c, o in zip(masks, counts, io):
        kept = np.flatnonzero(m)
        assert (o[:, 1] == c + len(kept)).all()
        assert np.array_equal(o[kept, 0], c + np.arange(len(kept)))
        assert np.array_equal(o[:, 0], c + np.cumsum(m) - m)                     # every lane: the kept ones before it


def test_best_hypothesis():
    rng = np.random.default_rng(32)
    its = [1, 64, 65, 4096, 4096, 4096, 4096, 130, 100]
    scores = rng.integers(0, 50, size=(len(its), 4096)).astype(np.int32)
    scores[4] = 17                                                       # all tie: the lowest h
    scores[5] = -1                                                       # none scored
    scores[6] = 3
    scores[6, [4095, 2049, 77 + 64 * 5]] = 40                          # ties across lanes and inside one lane
    scores[7, :130] = -5
    scores[7, 129] = 0
    for i, it in enumerate(its):
        scores[i, it:] = 10 ** 6                                         # past the end: must not be read
    got = DB.best_hypothesis(scores, its)
    for i, it in enumerate(its):
        s = scores[i, :it]
        best = int(s.max())
        assert (got[i, :, 0] == (best if best >= 0 else -1)).all(), i
        if best >= 0:
            assert (got[i, :, 1] == int(np.argmax(s))).all(), i
        else:
            assert (got[i, :, 0] < 0).all()
    refused = DB.best_hypothesis(scores[:2], [0, 4097])
    assert (refused[:, :, 0] == -2).all()


def test_sampler_matches_the_host_definition():
    rng = np.random.default_rng(33)
    x = np.r_[[0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], rng.integers(0, 2 ** 32, size=3000)].astype(np.uint32)
    _, io = DB.run("mix32", ix=x.view(np.int32))
    assert np.array_equal(io[:, 0].view(np.uint32), np.array([pnp._mix32(int(v)) for v in x], np.uint32))
    draws = np.c_[rng.integers(0, 2 ** 32, size=3000), rng.integers(1, 400, size=3000), rng.integers(0, 4096, size=3000),
                  rng.integers(0, 256, size=3000)]
    draws[:4, 1] = [1, 2, 2 ** 31 - 1, 368]
    _, io = DB.run("ransac_draw", ix=draws.astype(np.uint32).view(np.int32))
    want = np.array([pnp._ransac_draw(*map(int, d)) for d in draws])
    assert np.array_equal(io[:, 0], want) and (want >= 0).all() and (want < draws[:, 1]).all()
    # the sampler on one frame's ids: a full board, a board row (every triple collinear: None), and repeated ids
    rm1 = Z.BOARD[1] - 1
    for ids in (rng.permutation(Z.n_ids_of(Z.BOARD))[:129], np.arange(20) * rm1, np.r_[np.zeros(30, int), [5, 40, 77, 200]]):
        cases = np.c_[rng.integers(0, 2 ** 32, size=600), rng.integers(4, len(ids) + 1, size=600), rng.integers(0, 4096, size=600),
                      np.full(600, rm1)]
        got = DB.ransac_sample(ids, cases)
        for c, g in zip(cases, got):
            want = pnp._ransac_sample(int(c[0]), int(c[1]), int(c[2]), ids, rm1)
            assert (g[0] == 0) if want is None else (g[0] == 1 and g[1:].tolist() == list(want)), (c, g, want)
    assert (DB.ransac_sample(np.arange(10), [[1, 3, 0, rm1], [1, 11, 0, rm1]])[:, 0] == -1).all()
    # on_a_line over small grids, products past 2^31 included
    g = rng.integers(-3, 4, size=(2000, 8))
    g[:50] = rng.integers(-60000, 60000, size=(50, 8))
    g[50:60, 4:] = g[50:60, :4]                                        # the diagonal: always on a line
    abc = np.array([rng.permutation(4)[:3] for _ in range(len(g))])
    _, io = DB.run("on_a_line", ix=np.c_[g, abc])
    gx, gy, rows = g[:, :4].astype(object), g[:, 4:].astype(object), np.arange(len(g))
    a, b, c = abc.T
    want = (gx[rows, b] - gx[rows, a]) * (gy[rows, c] - gy[rows, a]) - (gy[rows, b] - gy[rows, a]) * (gx[rows, c] - gx[rows, a]) == 0
    assert np.array_equal(io[:, 0] != 0, want.astype(bool)) and want[50:60].all()


def test_unpk_is_the_inverse_of_pk():
    e = np.arange(-1, 140)
    _, io = DB.run("unpk", ix=e)
    for k, n in enumerate(DB.UNPK_N):
        ab = io[:, 2 * k:2 * k + 2]
        inside = (e >= 0) & (e < n * (n + 1) // 2)
        assert (ab[~inside] == -1).all()
        want = [(i, j) for i in range(n) for j in range(i, n)]
        assert ab[inside].tolist() == [list(w) for w in want], n
        ij = np.array([(i, j) for i in range(-1, n + 1) for j in range(-1, n + 1)])
        _, p = DB.run("pk", ix=ij)
        for (i, j), v in zip(ij, p[:, k]):
            if 0 <= i < n and 0 <= j < n:
                assert want[v] == (min(i, j), max(i, j))
            else:
                assert v == -1


# ------------------------------------------------------------------------------------------------ Gram and Schur

def test_accumulate_rows_and_lane_entries():
    rows, front, counts, starts = Z.gram_cases()
    acc, ea, eb, behind = DB.accumulate_rows(rows, front, counts, starts)
    want = [(i, j) for i in range(13) for j in range(i, 13)]
    print("\naccumulate_rows<13, 2, 13>")
    over = []
    for b, (n, s) in enumerate(zip(counts, starts)):
        e = np.arange(64)[:, None] + 64 * np.arange(2)[None, :]
        inside = e < 91
        assert (ea[b][~inside] == -1).all() and (eb[b][~inside] == -1).all()
        assert np.c_[ea[b][inside], eb[b][inside]].tolist() == [list(want[v]) for v in e[inside]]
        f = front[s:s + n]
        owns = np.zeros(64, int)
        owns[np.flatnonzero(f == 0) % 64] = 1
        assert np.array_equal(behind[b], owns)                           # the flag is the lane's own: the callers take __any of it
        got = np.zeros(91)
        got[e[inside]] = acc[b][inside]
        assert (acc[b][~inside] == 0.0).all()
        ref = Z.gram_reference(rows[s:s + n], f)
        d = np.sqrt(np.abs(cx.f64(Z.unpack(ref, 13)).diagonal()))
        d[d == 0] = 1.0
        scale = np.outer(d, d).astype(cx.LD)
        w = rows[s:s + n][f != 0].reshape(-1, 13)
        g_host = float((np.abs(Z.unpack(Z.pack(w.T @ w) - ref, 13)) / scale).max())
        g_dev = float((np.abs(Z.unpack(got - ref, 13)) / scale).max())
        if not _report("accumulate_rows", f"n = {n}{'' if f.all() else ', one row behind'}", g_host, g_dev):
            over.append(b)
    assert not over, over
    refused = DB.accumulate_rows(rows, front, [len(rows) + 1, 5, -1], [0, len(rows) - 4, 0])
    assert (refused[3] == -1).all()


@pytest.mark.parametrize("na", [6, 8, 9])
def test_schur_view(na):
    m = Z.schur_cases(na)
    sc, yz, ok = DB.schur_view(na, *m)
    assert (ok == 1).all()
    g_host, g_dev = HT.schur_host_gap(na), HT.schur_gap(na, m, sc, yz)
    print()
    assert _report(f"schur_view<{na}>", "random Grams", g_host, g_dev)
    bad = Z.schur_refusals(na)
    sc, yz, ok = DB.schur_view(na, *bad)
    assert (ok == 0).all() and not sc.any() and DB.untouched(yz).all()


# ------------------------------------------------------------------------------------------------ frames of a pool

def _status_ref(counts, starts, ids, pool, n_ids):
    out = []
    for n, s in zip(counts, starts):
        if n <= 0:
            out.append(pnp.PNP_TOO_FEW)
        elif s < 0 or s + n > pool:
            out.append(pnp.PNP_TRUNCATED)
        elif n < 4:
            out.append(pnp.PNP_TOO_FEW)
        else:
            out.append(pnp.PNP_BAD_ID if ((ids[s:s + n] < 0) | (ids[s:s + n] >= n_ids)).any() else pnp.PNP_OK)
    return out


def _overlap_ref(counts, starts, pool):
    rng_ = [(max(s, 0), min(s + n, pool)) if n > 0 else (0, 0) for n, s in zip(counts.astype(int), starts.astype(int))]
    return [int(lo < hi and any(o != b and olo < ohi and olo < hi and lo < ohi for o, (olo, ohi) in enumerate(rng_)))
            for b, (lo, hi) in enumerate(rng_)]


def test_frame_status_and_ranges_overlap():
    rng = np.random.default_rng(34)
    board = Z.BOARD
    nid = Z.n_ids_of(board)
    frame = lambda n: np.c_[rng.uniform(0, 300, size=(n, 2)), rng.choice(nid, n, replace=False)]
    frames = [frame(n) for n in (0, 1, 3, 4, 5, 63, 64, 65, 129, 70)]
    frames[5][62, 2] = nid                                             # a bad id in the last row of 63
    frames[7][64, 2] = -1                                              # a bad id in the second chunk of 65
    pool = 380
    packed, _ = pool_cases.lay_frames(frames, pool, gap=1)              # the last frame runs past the pool's end
    counts, starts, rows, xy, _ = corner_pool.views(packed, len(frames), pool)
    got = DB.frame_checks(counts, starts, rows, xy, pool, board)
    assert Z.same_bits(got.astype(np.float64), np.repeat(got[:, :1], 64, 1).astype(np.float64))
    assert got[:, 0, 0].tolist() == _status_ref(counts, starts, rows[:, 2], pool, nid)
    assert got[:, 0, 0].tolist() == [pnp.PNP_TOO_FEW] * 3 + [pnp.PNP_OK] * 2 + [pnp.PNP_BAD_ID, pnp.PNP_OK, pnp.PNP_BAD_ID, pnp.PNP_OK,
                                                                                  pnp.PNP_TRUNCATED]
    assert np.array_equal(got[:, 0, 1], counts) and np.array_equal(got[:, 0, 2], starts)
    assert got[:, 0, 3].tolist() == _overlap_ref(counts, starts, pool) == [0] * len(frames)
    # hand-laid ranges: shared slots, a range inside another, negative starts, empty frames, ranges that only touch
    counts = np.array([10, 10, 4, 0, 6, 5, 5, 8, 3], np.int32)
    starts = np.array([0, 9, 30, 2, -3, 40, 45, 96, 120], np.int32)
    pool = 100
    got = DB.frame_checks(counts, starts, np.zeros((pool, 4), np.int32), None, pool, board)
    assert got[:, 0, 3].tolist() == _overlap_ref(counts, starts, pool) == [1, 1, 0, 0, 1, 0, 0, 0, 0]
    assert (got[:, :, 3] == got[:, :1, 3]).all()
    assert got[:, 0, 0].tolist() == _status_ref(counts, starts, np.zeros(pool, int), pool, nid)
    # 70 views: the other views are shared out over more than one pass of the 64 lanes
    counts = np.full(70, 2, np.int32)
    starts = (np.arange(70) * 2).astype(np.int32)
    starts[69] = 131                                                   # view 69 shares slot 132 with view 66 and 131 with 65
    got = DB.frame_checks(counts, starts, np.zeros((200, 4), np.int32), None, 200, board)
    assert got[:, 0, 3].tolist() == _overlap_ref(counts, starts, 200)
    assert got[[65, 66, 69], 0, 3].tolist() == [1, 1, 1] and got[:, 0, 3].sum() == 3


@pytest.mark.parametrize("which", ["pinhole-none", "pinhole-8", "fisheye"])
def test_frame_blocks(which):
    fs = Z.fisheye_frame_set() if which == "fisheye" else Z.pinhole_frame_set(which.split("-")[1])
    pool = sum(len(k) for k in fs.kps) + 3
    packed, _ = pool_cases.lay_frames(fs.kps, pool, first=2)
    counts, starts, rows, xy, _ = corner_pool.views(packed, len(fs.kps), pool)
    out, io = DB.frame_blocks(fs.model, counts, starts, rows, xy, pool, fs.board, fs.camera, fs.poses)
    # all 64 lanes hold the same bits, of every output and every verdict
    assert Z.same_bits(out, np.repeat(out[:, :1], 64, 1))
    assert (io == io[:, :1]).all()
    out, io = out[:, 0], io[:, 0]
    O, I = DB.FRAME_OUT, DB.FRAME_IOUT
    n = len(fs.refs)
    assert (io[:n, I["readable"]] == 1).all() and (io[:n, I["inside"]] == 1).all()
    assert (io[:n, [I["st_H"], I["st_init"], I["st_solve"]]] == pnp.PNP_OK).all()
    res = [(o[O["H"]], o[O["mc"]], o[O["p0"]], o[O["acc"]]) for o in out[:n]]
    host_res = HT.host_frame_results(fs)
    host, dev = HT.frame_gaps(fs, host_res), HT.frame_gaps(fs, res)
    print(f"\n{fs.name}")
    ok = True
    for zone in host:
        for label, gh, gd in zip(("homography", "init_pose", "evaluate"), host[zone], dev[zone]):
            ok &= _report(label, f"{fs.name}, {zone}", gh, gd)
    assert ok
    tally = [0, 0, 0]
    K, k = HT._K(fs.camera), fs.camera[4:]
    for ref, o, r, h in zip(fs.refs, out[:n], res, host_res):
        assert HT.truth_gap(r[2], ref["truth"]) <= HT.TRUTH_BOUND
        assert Z.pose_gap(r[2], (cx.rotation(h[2][:3]), h[2][3:].astype(cx.LD))) <= 1e-4                  # against pnp._init_pose itself
        assert abs(o[O["cost"]] - o[O["acc"]][0]) <= Z.gate(0.0) * o[O["cost"]]                            # evaluate<false>'s cost is evaluate<true>'s
        if fs.model == "pinhole":
            st, pose = pnp._solve(ref["obj"].astype(np.float32), ref["img"].astype(np.float32), K, k)
        else:
            from deepcharuco_amd import fisheye
            st, pose = fisheye._solve(ref["obj"].astype(np.float32), ref["img"].astype(np.float32), K, k)
        assert st == pnp.PNP_OK
        _agree_rot(o[O["pose"]], pose, tally)
    print(f"  solve against the host's: {tally[0]} within 1e-9, {tally[1]} within 1e-6 at the same cost, {tally[2]} at the step cap")
    # four rows: the DLT homography against the closed form through the same four points
    for i in range(n):
        if len(fs.kps[i]) == 4 and fs.model == "pinhole":
            mn, _ = DB.run("undistort", np.c_[np.tile(fs.camera, (4, 1)), fs.refs[i]["img"]])
            h4, st = DB.run("homography4", np.r_[fs.refs[i]["obj"][:, 0], fs.refs[i]["obj"][:, 1], mn[:, 0], mn[:, 1]][None])
            assert st[0, 0] == pnp.PNP_OK
            g4 = Z.homography_gap(h4[0, :9], h4[0, 9:], fs.refs[i]["H"])
            gd = Z.homography_gap(res[i][0], res[i][1], fs.refs[i]["H"])
            gh = Z.homography_gap(host_res[i][0], host_res[i][1], fs.refs[i]["H"])
            print(f"  four rows ({fs.zones[i]}): DLT {gd:.2e}, closed form {g4:.2e} against the exact homography through them")
            assert g4 <= Z.gate(gh) and np.abs(h4[0, :9] - res[i][0]).max() <= 2 * Z.gate(gh) * np.abs(res[i][0]).max()
    # the extras
    x = fs.extras
    if fs.model == "pinhole":
        b = x["behind"]
        assert np.isposinf(out[b, O["acc"]][0]) and np.isposinf(out[b, O["cost"]]) and io[b, I["st_H"]] == pnp.PNP_OK
        for name in ("collinear ids", "coincident image"):
            b = x[name]
            assert io[b, I["st_H"]] == io[b, I["st_init"]] == io[b, I["st_solve"]] == pnp.PNP_DEGENERATE, name
            assert DB.untouched(out[b, 29:]).all(), name
        b = x["bad id"]
        assert io[b, 0] == -100 and (io[b, 1:] == DB.IFILL).all() and DB.untouched(out[b]).all()
    else:
        b = x["outside"]
        assert io[b, I["inside"]] == 0 and (io[b, 1:4] == DB.IFILL).all() and DB.untouched(out[b, 29:]).all()


# ------------------------------------------------------------------------------------------------ under graph replay

def test_three_launchers_replay_to_the_eager_bits():
    zr = Z.rodrigues_zones()[6]
    zj = Z.eigen_reference(9, Z.JACOBI9_COUNT)["DLT normal matrices"][0]
    xj = np.array([Z.pack(A) for A in zj])
    xw = Z.reduction_inputs(64, 28, 8).reshape(8, -1)
    jobs = [("rodrigues", zr.x, 1), ("jacobi9", xj, 64), ("wave_sum28", xw, 64)]
    eager = [DB.run(name, x)[0] for name, x, _ in jobs]
    bufs = []
    for name, x, lanes in jobs:
        _, nin, niin, nout, niout = DB.BLOCKS[name]
        n = len(x)
        bufs.append((DB.to_dev(x, np.float64), DB.to_dev(np.zeros(n * niin), np.int32), DB.filled(n * lanes * nout, np.float64),
                     DB.filled(n * lanes * niout, np.int32), n))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                         # (a first run outside the capture)
        for (name, _, _), b in zip(jobs, bufs):
            assert DB.launch(name, *b) == 0
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for b in bufs:
        b[2].copy_(DB.filled(b[2].numel(), np.float64))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for (name, _, _), b in zip(jobs, bufs):
            assert DB.launch(name, *b) == 0
    torch.cuda.synchronize()
    assert all(DB.untouched(b[2].cpu().numpy()).all() for b in bufs)   # capture ran nothing
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    for e, b in zip(eager, bufs):
        assert Z.same_bits(b[2].cpu().numpy().reshape(e.shape), e)
