"""The host definition of the RANSAC pose solver (deepcharuco_amd/pnp.py, solve_pnp_ransac_host_full): the integer sampler, frames
with planted wrong ids, clean frames, duplicate ids, every status and the refused arguments.  No GPU needed.

The planted-outlier frames are also what tests/test_gpu_pnp_ransac.py runs on the device; their margins (how far the nearest
row of any near-winning hypothesis is from the inlier threshold, relative) are asserted here to be >= 1e-6, which is what lets
that file demand equal masks and winners from a kernel that agrees with this definition to ~1e-9."""
import itertools

import numpy as np
import pytest

from deepcharuco_amd import pnp
from test_pnp_host import BOARD, DIST5, K, make_frame

RM1 = BOARD[1] - 1
PLANTED_SEED, SAMPLER_SEED, REPROJ = 2025, 7, 3.0
N_CORNERS = [16, 16, 12, 10, 9, 16, 14, 12]
N_WRONG = [3, 5, 3, 2, 2, 0, 4, 1]


def planted_frames(count=32):
    """-> list of (keypoints with wrong ids planted, good-row mask, true pose[6]): seeded sigma = 0.3 px views of the 5x5 board;
    a wrong id is another id of the board."""
    rng = np.random.default_rng(PLANTED_SEED)
    out = []
    for b in range(count):
        n, n_wrong = N_CORNERS[b % 8], N_WRONG[b % 8]
        ids = np.sort(rng.choice(16, n, replace=False))
        kp, r, t = make_frame(rng, ids=ids, sigma=0.3)
        bad = rng.choice(n, n_wrong, replace=False)
        for j in bad:
            kp[j, 2] = (kp[j, 2] + rng.integers(1, 16)) % 16
        good = np.ones(n, bool)
        good[bad] = False
        out.append((kp, good, np.r_[r, t]))
    return out


def _ransac(kp, **kw):
    args = dict(iterations=100, reproj_error=REPROJ, min_inliers=4, seed=SAMPLER_SEED)
    args.update(kw)
    return pnp.solve_pnp_ransac_host_full(kp, *BOARD, K, DIST5, **args)


# ------------------------------------------------------------------------------------------------ the sampler

def test_sampler_gives_four_distinct_slots_in_range():
    for seed, ids, rm1 in ((0, [0, 1, 4, 5], RM1), (7, [0, 1, 4, 5, 10], RM1), (7, np.arange(16), RM1), (99, np.arange(300), 19)):
        n = len(ids)
        got = 0
        for h in range(200):
            s = pnp._ransac_sample(seed, n, h, ids, rm1)
            if s is None:
                continue
            got += 1
            assert len(s) == 4 and len(set(s)) == 4 and all(0 <= i < n for i in s)
            assert pnp._ransac_sample_ok([int(ids[i]) for i in s], rm1)
        assert got >= 150, (n, got)
    assert all(0 <= pnp._ransac_draw(s, n, h, c) < n for s in (0, 2 ** 32 - 1) for n in (1, 4, 7, 2 ** 20) for h in (0, 4095)
               for c in range(64))


def test_sampler_literal_values():
    """A later edit of the hash or of the redraw order shows here (the kernel restates both)."""
    assert pnp._mix32(1) == 1753845952 and pnp._mix32(0xDEADBEEF) == 3861431939
    assert [pnp._ransac_draw(7, 16, h, c) for h in range(3) for c in range(4)] == [10, 15, 14, 6, 6, 10, 15, 5, 3, 2, 4, 2]
    assert [pnp._ransac_draw(0, 300, 99, c) for c in range(4)] == [14, 163, 2, 202]
    assert pnp._ransac_draw(2 ** 32 + 7, 16, 0, 0) == 10                       # the seed is taken modulo 2^32
    want = {(0, 16, 0): [5, 15, 4, 12], (0, 16, 1): [12, 15, 7, 2],
            (7, 16, 0): [6, 14, 4, 3],                                         # its first draw (10, 15, 14, 6) holds a column triple
            (7, 16, 5): [6, 10, 5, 1], (7, 9, 5): [8, 7, 2, 1]}
    for (seed, n, h), s in want.items():
        assert pnp._ransac_sample(seed, n, h, np.arange(n), RM1) == s
    assert pnp._ransac_sample(123456789, 300, 4095, np.arange(300), 19) == [53, 229, 18, 293]


def test_sample_refusals_are_exact_on_the_id_grid():
    ok = pnp._ransac_sample_ok
    assert ok([0, 1, 4, 5], RM1) and ok([0, 3, 12, 15], RM1) and ok([1, 4, 6, 9], RM1) and ok([0, 2, 7, 13], RM1)
    assert not ok([0, 1, 4, 4], RM1) and not ok([5, 5, 5, 5], RM1)                 # a shared id
    assert not ok([0, 1, 2, 7], RM1) and not ok([7, 0, 1, 2], RM1)                 # three of a board row, wherever they stand
    assert not ok([1, 5, 9, 14], RM1) and not ok([0, 5, 10, 3], RM1) and not ok([3, 6, 9, 0], RM1)   # column, both diagonals
    assert not ok([0, 6, 12, 1], 5) and ok([0, 6, 12, 1], RM1)                      # the grid is (id % rm1, id // rm1)
    assert not ok([0, 9, 18, 5], 8)                                                 # (0,0) (1,1) (2,2)
    assert not ok([0, 10, 20, 1], 8)                                                # (0,0) (2,1) (4,2): slope 1/2
    # 542 of the 1,820 4-subsets of the 4x4 grid hold a collinear triple
    assert sum(not ok(list(c), RM1) for c in itertools.combinations(range(16), 4)) == 542


def test_sampler_on_hand_built_id_sets():
    # every 4-subset of these rows holds three ids of one board row: no hypothesis
    assert all(pnp._ransac_sample(7, 5, h, [0, 1, 2, 3, 5], RM1) is None for h in range(50))
    # two distinct ids only
    assert all(pnp._ransac_sample(7, 6, h, [3, 3, 3, 7, 7, 7], RM1) is None for h in range(50))
    # a unit square with one id twice: the sample is the square, through either copy
    ids, seen = [0, 1, 4, 5, 5], set()
    for h in range(100):
        s = pnp._ransac_sample(7, 5, h, ids, RM1)
        if s is not None:
            assert sorted(ids[i] for i in s) == [0, 1, 4, 5]
            seen.add(tuple(sorted(s)))
    assert seen == {(0, 1, 2, 3), (0, 1, 2, 4)}


def test_sampler_depends_on_seed_n_h_and_the_ids_only():
    ids = np.arange(16)
    a = [pnp._ransac_sample(7, 16, h, ids, RM1) for h in range(40)]
    assert a == [pnp._ransac_sample(7, 16, h, ids.copy(), RM1) for h in range(40)]
    assert a != [pnp._ransac_sample(8, 16, h, ids, RM1) for h in range(40)]
    assert a[:12] != [pnp._ransac_sample(7, 12, h, ids[:12], RM1) for h in range(12)]
    # the ids enter through the refusals only: where the first four distinct draws are accepted, they are the sample
    for h in range(40):
        first = [pnp._ransac_draw(7, 16, h, c) for c in range(8)]
        distinct = list(dict.fromkeys(first))[:4]
        if pnp._ransac_sample_ok([int(ids[i]) for i in distinct], RM1):
            assert a[h] == distinct
    # the hypotheses of a frame are the same whatever else is solved with it: the definition takes one frame and no batch index
    kp = planted_frames(1)[0][0]
    assert _ransac(kp)[3] == _ransac(kp.copy())[3]


# ------------------------------------------------------------------------------------------------ frames

def test_planted_wrong_ids_are_found_in_every_frame():
    worst_margin, report = np.inf, []
    for b, (kp, good, truth) in enumerate(planted_frames()):
        st, pose, mask, winner, margin = _ransac(kp, with_margin=True)
        assert st == pnp.PNP_OK, (b, st)
        assert mask.dtype == bool and np.array_equal(mask, good), (b, mask, good)
        st_good, pose_good = pnp.solve_pnp_host_full(kp[good], *BOARD, K, DIST5)
        assert st_good == pnp.PNP_OK and np.array_equal(pose, pose_good), (b, pose, pose_good)      # same function, same rows
        assert 0 <= winner < 100 and margin >= 1e-6, (b, winner, margin)
        worst_margin = min(worst_margin, margin)
        terr = np.linalg.norm(pose[3:6] - truth[3:]) / np.linalg.norm(truth[3:])
        if not good.all():          # the point of the feature: the plain least-squares fit over every row is worse
            st_plain, pose_plain = pnp.solve_pnp_host_full(kp, *BOARD, K, DIST5)
            terr_plain = np.linalg.norm(pose_plain[3:6] - truth[3:]) / np.linalg.norm(truth[3:]) if st_plain == pnp.PNP_OK else np.inf
            assert terr_plain > terr, (b, terr_plain, terr)
            report.append((terr_plain, terr))
    print("smallest margin %.3g; translation error plain %.3g..%.3g, ransac %.3g..%.3g" % (
        worst_margin, min(r[0] for r in report), max(r[0] for r in report), min(r[1] for r in report), max(r[1] for r in report)))


def test_clean_frames_keep_every_row_and_the_plain_pose():
    rng = np.random.default_rng(31)
    for i in range(8):
        kp, _, _ = make_frame(rng, sigma=0.3 if i % 2 else 0.0)
        kp = kp[rng.permutation(16)]                                     # caller's row order: not id-sorted
        st, pose, mask, winner = _ransac(kp, reproj_error=8.0)
        assert st == pnp.PNP_OK and mask.all() and mask.shape == (16,) and winner >= 0
        st0, pose0 = pnp.solve_pnp_host_full(kp[np.argsort(kp[:, 2], kind="stable")], *BOARD, K, DIST5)
        assert st0 == pnp.PNP_OK and np.array_equal(pose, pose0)
        ret, rvec, tvec, inl = pnp.solve_pnp_ransac_host(kp, *BOARD, K, DIST5, seed=SAMPLER_SEED)
        assert ret is True and rvec.shape == (3, 1) and tvec.shape == (3, 1) and rvec.dtype == np.float64
        assert np.array_equal(np.r_[rvec.ravel(), tvec.ravel()], pose[:6]) and np.array_equal(inl, mask)


def test_mask_is_in_the_callers_row_order():
    kp, good, _ = planted_frames(1)[0]
    perm = np.random.default_rng(1).permutation(len(kp))
    st, pose, mask, winner = _ransac(kp)
    st_p, pose_p, mask_p, winner_p = _ransac(kp[perm])
    assert st == st_p == pnp.PNP_OK and winner == winner_p and np.array_equal(pose, pose_p)       # distinct ids: one sorted order
    assert np.array_equal(mask_p, good[perm])


def test_pool_order_takes_the_rows_as_they_stand():
    """A pool need not be id-sorted (infer_batch_device leaves raster order); the sampler's slots count the pool's rows."""
    kp, good, _ = planted_frames(1)[0]
    srt = kp[np.argsort(kp[:, 2], kind="stable")]
    a, b = _ransac(srt), _ransac(srt, pool_order=True)
    assert a[0] == b[0] and a[3] == b[3] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])    # sorted rows: the same
    perm = np.random.default_rng(2).permutation(len(kp))
    st, pose, mask, winner, margin = _ransac(kp[perm], pool_order=True, with_margin=True)
    assert st == pnp.PNP_OK and margin >= 1e-6 and np.array_equal(mask, good[perm])      # other samples, the same consensus
    s = pnp._ransac_sample(SAMPLER_SEED, len(kp), winner, kp[perm][:, 2].astype(int), RM1)
    assert s is not None and mask[s].all()                                               # drawn from the rows as given


def test_duplicate_ids_the_displaced_copy_is_out():
    rng = np.random.default_rng(7)
    ids = np.array([0, 3, 3, 5, 6, 9, 12, 15, 15])
    kp, r, t = make_frame(rng, ids=ids)
    kp[2, :2] += (9.0, -7.0)                 # one copy of id 3 sits 11 px from its corner
    kp[8, :2] += (-6.0, 8.0)                 # one copy of id 15 too
    st, pose, mask, _ = _ransac(kp)
    want = np.ones(9, bool)
    want[[2, 8]] = False
    assert st == pnp.PNP_OK and np.array_equal(mask, want)
    assert np.linalg.norm(pose[:3] - r) <= 1e-4 * np.linalg.norm(r) and np.linalg.norm(pose[3:6] - t) <= 1e-4 * np.linalg.norm(t)


def test_every_status():
    kp, good, _ = planted_frames(1)[0]
    for n in (0, 1, 3):
        st, pose, mask, winner = _ransac(kp[:n])
        assert st == pnp.PNP_TOO_FEW and not pose.any() and mask.shape == (n,) and not mask.any() and winner == -1
    assert _ransac(np.array([]))[0] == pnp.PNP_TOO_FEW
    ret, rvec, tvec, inl = pnp.solve_pnp_ransac_host(kp[:3], *BOARD, K, DIST5)
    assert ret is False and rvec is None and tvec is None and inl.shape == (3,) and not inl.any()
    # more inliers asked for than any hypothesis reaches
    st, pose, mask, winner, margin = _ransac(kp, min_inliers=int(good.sum()) + 1, with_margin=True)
    assert st == pnp.PNP_NO_CONSENSUS == 6 and not pose.any() and not mask.any() and mask.shape == good.shape and winner >= 0
    assert np.isfinite(margin)
    assert _ransac(kp, min_inliers=int(good.sum()))[0] == pnp.PNP_OK
    assert _ransac(kp, min_inliers=-3)[0] == pnp.PNP_OK                      # the floor is four
    # all rows on one board line: no sample passes the sampler
    for ids in ([0, 1, 2, 3], [0, 5, 10, 15], [1, 5, 9, 13, 1]):
        kpc, _, _ = make_frame(np.random.default_rng(5), ids=ids)
        st, pose, mask, winner = _ransac(kpc)
        assert st == pnp.PNP_DEGENERATE and not pose.any() and not mask.any() and winner == -1
        assert pnp.solve_pnp_ransac_host(kpc, *BOARD, K, DIST5)[0] is False
    # one iteration is allowed, and is then the only hypothesis
    st, _, mask, winner = _ransac(kp, iterations=1)
    assert winner in (0, -1) and (st == pnp.PNP_DEGENERATE) == (winner == -1)


def test_refused_arguments():
    kp = planted_frames(1)[0][0]
    for kw in (dict(iterations=0), dict(iterations=4097), dict(reproj_error=0.0), dict(reproj_error=-1.0),
               dict(reproj_error=np.inf), dict(reproj_error=np.nan)):
        with pytest.raises(ValueError):
            _ransac(kp, **kw)
    with pytest.raises(ValueError):
        pnp.solve_pnp_ransac_host(kp, *BOARD, K, np.zeros(12))
    skew = K.copy()
    skew[0, 1] = 1.0
    with pytest.raises(ValueError):
        pnp.solve_pnp_ransac_host(kp, *BOARD, skew, DIST5)
    bad = kp.copy()
    bad[0, 2] = 16
    with pytest.raises(IndexError):
        pnp.solve_pnp_ransac_host(bad, *BOARD, K, DIST5)
    assert _ransac(kp, iterations=4096, reproj_error=1e-3)[0] in (pnp.PNP_OK, pnp.PNP_NO_CONSENSUS)
