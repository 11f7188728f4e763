"""CPU: the numpy restatement of the staged C ABI's index contracts (tests/staged_exact.py) against the oracle's stage functions,
its truncation laws, and the staged entries' refusals that need no GPU.  tests/test_gpu_staged_abi.py compares the kernels with
the restatement."""
import numpy as np
import pytest
import torch

from oracle import deepcharuco_oracle as O
from staged_exact import SENTINEL, decode_rows, gather_u8, patch_table

SHAPES = [(1, 1), (8, 12), (30, 40), (31, 41)]


def _seeded_maps(seed, hc, wc, n_ids, dust_bin):
    """Four frames of label maps as pred_argmax returns them: random, nothing fires, everything fires, sparse."""
    rng = np.random.default_rng([seed, hc, wc])
    loc = rng.integers(0, 65, (4, hc, wc))
    ids = rng.integers(0, n_ids + 1, (4, hc, wc))
    ids[1] = dust_bin
    ids[2] = np.where(ids[2] == dust_bin, (dust_bin + 1) % (n_ids + 1), ids[2])
    loc[2] = np.minimum(loc[2], 63)
    ids[3] = np.where(rng.random((hc, wc)) < 0.9, dust_bin, ids[3])
    return loc, np.where(loc == 64, dust_bin, ids)


@pytest.mark.parametrize("hw", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
@pytest.mark.parametrize("n_ids,dust_bin", [(16, 16), (16, 3), (40, 40), (8, 0)])
def test_decode_rows_equals_the_oracle(hw, n_ids, dust_bin):
    hc, wc = hw
    loc, ids = _seeded_maps(5, hc, wc, n_ids, dust_bin)
    cells = hc * wc
    counts, rows = decode_rows(loc, ids, dust_bin, cells)
    assert counts[1] == 0 and counts[2] == cells
    kp, idf = O.label_to_keypoints(torch.from_numpy(loc), torch.from_numpy(ids), dust_bin)
    cat = np.concatenate([rows[f, :counts[f]] for f in range(4)])
    assert np.array_equal(cat[:, :2], kp.numpy()) and np.array_equal(cat[:, 2], idf.numpy())
    for f in range(4):                          # per frame too, and the cell index against torch.nonzero's
        kf, idf_f = O.label_to_keypoints(torch.from_numpy(loc[f:f + 1]), torch.from_numpy(ids[f:f + 1]), dust_bin)
        r = rows[f, :counts[f]]
        assert np.array_equal(r[:, :2], kf.numpy()) and np.array_equal(r[:, 2], idf_f.numpy())
        nz = torch.nonzero(torch.from_numpy(ids[f]) != dust_bin).numpy()
        assert np.array_equal(r[:, 3], nz[:, 0] * wc + nz[:, 1])
        assert np.all(rows[f, counts[f]:] == SENTINEL)


@pytest.mark.parametrize("hw", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_decode_rows_equals_the_oracle_from_logits(hw):
    """pred_to_keypoints on seeded logits (ties and class 64 winners included) == decode_rows of pred_argmax's maps."""
    hc, wc = hw
    rng = np.random.default_rng([9, hc, wc])
    loc_hat = torch.from_numpy(rng.integers(-3, 4, (3, 65, hc, wc)).astype(np.float32))      # small integers: many exact ties
    ids_hat = torch.from_numpy(rng.integers(-3, 4, (3, 17, hc, wc)).astype(np.float32))
    loc_hat[:, 64] += 2.0
    for dust_bin in (16, 3):
        la, ia = O.pred_argmax(loc_hat, ids_hat, dust_bin)
        counts, rows = decode_rows(la.numpy(), ia.numpy(), dust_bin, hc * wc)
        kp, idf = O.pred_to_keypoints(loc_hat, ids_hat, dust_bin)
        cat = np.concatenate([rows[f, :counts[f]] for f in range(3)])
        assert np.array_equal(cat[:, :2], kp.numpy()) and np.array_equal(cat[:, 2], idf.numpy())
        if hc * wc > 50:
            assert int((la == 64).sum()) > 0 and int(counts.sum()) > 0


def _border_keypoints(h, w):
    pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2),
           (min(11, w - 1), min(11, h - 1)), (min(12, w - 1), min(12, h - 1)), (w // 2, h // 2), (w // 3, 2 * h // 3)]
    return np.array(pts, np.int64)


@pytest.mark.parametrize("hw", [(8, 8), (9, 15), (40, 56), (64, 96)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_gather_u8_equals_the_oracle(hw):
    h, w = hw
    rng = np.random.default_rng([3, h, w])
    frames = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    frames[0, 0, 0], frames[0, -1, -1] = 0, 255
    kp = _border_keypoints(h, w)
    for f in range(3):
        table = np.zeros((len(kp), 4), np.int32)
        table[:, 0], table[:, 1:3], table[:, 3] = f, kp, np.arange(len(kp))
        got = gather_u8(frames, table)
        exp = O.extract_patches(torch.from_numpy(O.pre_bgr_image(frames[f])), torch.from_numpy(kp)).numpy()
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    if h < 12 and w < 24:                       # smaller than a patch: every patch has zero padding
        assert np.all((got == 0).reshape(len(kp), -1).any(axis=1))


def test_truncation_laws():
    """kmax = k is kmax = infinity cut to k rows per frame; the counts do not change; total and the slots follow."""
    hc, wc = 8, 12
    loc, ids = _seeded_maps(11, hc, wc, 16, 16)
    cells = hc * wc
    c_inf, r_inf = decode_rows(loc, ids, 16, cells)
    t_inf, n_inf = patch_table(c_inf, r_inf, cells)
    assert n_inf == int(c_inf.sum()) and c_inf.max() == cells and c_inf.min() == 0
    for k in (1, 2, 7, max(1, int(c_inf[3])), int(c_inf[3]) + 1, cells - 1, cells, cells + 5):
        c, r = decode_rows(loc, ids, 16, k)
        assert np.array_equal(c, c_inf)
        kept = np.minimum(c_inf, k)
        for f in range(4):
            assert np.array_equal(r[f, :kept[f]], r_inf[f, :kept[f]]) and np.all(r[f, kept[f]:] == SENTINEL)
        t, n = patch_table(c, r, k)
        assert n == int(kept.sum()) and t.shape == (n, 4)
        exp = np.concatenate([np.column_stack([np.full(kept[f], f), r_inf[f, :kept[f], :2], f * k + np.arange(kept[f])])
                              for f in range(4)])
        assert np.array_equal(t, exp)
        assert len(set(t[:, 3].tolist())) == n and (n == 0 or t[:, 3].max() < 4 * k)
    t0, n0 = patch_table(np.zeros(3, np.int32), np.full((3, 5, 4), SENTINEL, np.int32), 5)
    assert n0 == 0 and t0.shape == (0, 4)


def test_staged_entries_refuse_null_arguments_without_a_gpu():
    from deepcharuco_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(64, np.int32)               # a non-null HOST address: every call below is refused before it is used
    p = buf.ctypes.data
    assert lib.dcx_detector_decode(None, 1, 64, 96, p, 16, 96, p, p, None, None, None) == -1
    assert lib.dcx_build_patch_table(None, p, 1, 4, p, p, None) == -1
    assert lib.dcx_build_patch_table(p, None, 1, 4, p, p, None) == -1
    assert lib.dcx_build_patch_table(p, p, 1, 4, None, p, None) == -1
    assert lib.dcx_build_patch_table(p, p, 1, 4, p, None, None) == -1
    assert lib.dcx_extract_patches_u8(None, 64 * 96, 96, 64, 96, p, None, 1, p, None) == -1
    assert lib.dcx_extract_patches_u8(p, 64 * 96, 96, 64, 96, None, None, 1, p, None) == -1
    assert lib.dcx_extract_patches_u8(p, 64 * 96, 96, 64, 96, p, None, 1, None, None) == -1
    assert lib.dcx_extract_patches_f32(None, 64, 96, p, None, 1, p, None) == -1
    assert lib.dcx_extract_patches_f32(p, 64, 96, None, None, 1, p, None) == -1
    assert lib.dcx_extract_patches_f32(p, 64, 96, p, None, 1, None, None) == -1
    assert lib.dcx_label_to_keypoints(None, p, 1, 8, 12, 16, 96, p, p, p, None, None) == -1
    assert lib.dcx_label_to_keypoints(p, None, 1, 8, 12, 16, 96, p, p, p, None, None) == -1
    assert lib.dcx_label_to_keypoints(p, p, 1, 8, 12, 16, 96, None, p, p, None, None) == -1
    assert lib.dcx_label_to_keypoints(p, p, 1, 8, 12, 16, 96, p, None, p, None, None) == -1
    assert lib.dcx_label_to_keypoints(p, p, 1, 8, 12, 16, 96, p, p, None, None, None) == -1
    assert lib.dcx_pred_to_keypoints(None, p, 1, 65, 17, 8, 12, 16, 96, p, p, None, None, None) == -1
    assert lib.dcx_refiner_forward(None, p, 1, None, None, p, 1 << 20, p, None, None, None) == -1
