"""Host (no GPU) anchor of the chained exact restatement (oracle/net_exact.py).

The restatement is read off the kernels' summation orders; the GPU tests (test_gpu_exact_chain.py) compare the HIP path with it
bit for bit.  This file ties it to the maths: the same networks evaluated in float64 by the oracle graph
(oracle/deepcharuco_oracle.py), and the committed fixtures made by the reference itself."""
import numpy as np
import pytest
import torch

from oracle import deepcharuco_oracle as O
from oracle import net_exact as N

LOGIT_ATOL = 5e-5       # the gate of the golden comparisons (test_gpu_parity.py)
F64_ATOL = 2e-5         # restated fp32 chain vs float64: the largest measured is 1.4e-5 (deterministic mode, 64x96 frame)
# Heat-map logits: the head is a raw 1x1 over 64 BN + ReLU channels after eleven conv layers, the same depth and kind of chain as
# the detector's logits, and the heat stays in the logits' range (|heat| <= 3.3 on the fixture's patches against |logit| <= ~6),
# so fp32 rounding accumulates to the same size: the logits' bound holds (the largest measured is 8.7e-6).
HEAT_F64_ATOL = 2e-5
ARGMAX_MARGIN = 1e-4    # arg-max decisions must agree wherever the float64 top-2 gap is wider than this


@pytest.fixture(scope="module")
def case():
    from conftest import GoldenCase
    return GoldenCase("tiny_noise_64x96")


def _f64(sd):
    return {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in sd.items()}


def _top2_gap(a, axis):
    s = np.sort(a, axis=axis)
    return np.take(s, -1, axis=axis) - np.take(s, -2, axis=axis)


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
def test_detector_restatement_vs_float64_and_golden(case, deterministic):
    x = O.pre_bgr_image(case.frame)
    l64, i64 = [t.numpy() for t in O.detector_forward(_f64(case.sd_dc), torch.from_numpy(x).double()[None])]
    loc, ids = N.detector_exact(case.sd_dc, case.frame[None], deterministic=deterministic)
    assert loc.dtype == np.float32 and loc.shape == l64.shape and ids.shape == i64.shape
    assert np.abs(loc - l64).max() <= F64_ATOL and np.abs(ids - i64).max() <= F64_ATOL
    for got, ref in ((loc, l64), (ids, i64)):
        safe = _top2_gap(ref, 1) > ARGMAX_MARGIN
        assert safe.sum() >= 0.9 * safe.size
        assert np.array_equal(got.argmax(1)[safe], ref.argmax(1)[safe])
    assert np.abs(loc[0] - case.fx["loc_logits"]).max() <= LOGIT_ATOL
    assert np.abs(ids[0] - case.fx["ids_logits"]).max() <= LOGIT_ATOL
    # the u8 / f32 / BGR entries of the restatement are one and the same chain
    bgr = np.repeat(case.frame[None, ..., None], 3, axis=3)
    for frames, pix in ((x, "f32"), (bgr, "bgr"), (bgr, "legacy14")):
        l2, i2 = N.detector_exact(case.sd_dc, frames, pix=pix, deterministic=deterministic)
        assert np.array_equal(l2, loc) and np.array_equal(i2, ids)


def test_detector_families_follow_the_rule():
    fams = {d: [f for _, f, _ in N.detector_layers(1, 64, 96, 16, d)] for d in (False, True)}
    assert fams[True] == ["direct"] * 10
    assert fams[False] == ["w2h"] * 8 + ["direct"] * 2
    rfams = [f for _, f, _ in N.refinenet_layers(1, False)]
    assert rfams == ["w2h"] * 5 + ["w2p", "w2h", "w2p", "w2h", "w2p"]
    assert [f for _, f, _ in N.refinenet_layers(1, True)] == ["direct"] * 10


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
def test_refinenet_restatement_vs_float64_and_golden(case, deterministic):
    x = torch.from_numpy(O.pre_bgr_image(case.frame))
    patches = O.extract_patches(x, torch.from_numpy(case.fx["kpts"])).numpy()
    h64 = O.refinenet_forward(_f64(case.sd_rn), torch.from_numpy(patches).double()[:, None]).numpy()
    body = N.refinenet_body(case.sd_rn, patches, deterministic)
    heats = {}
    for order in ("direct", "w2p"):
        heat = N.refinenet_head(case.sd_rn, body, order)
        heats[order] = heat
        assert heat.dtype == np.float32 and heat.shape == h64.shape
        assert np.abs(heat - h64).max() <= HEAT_F64_ATOL
        assert np.abs(heat[:2, 0] - case.fx["heat_first2"]).max() <= LOGIT_ATOL
        flat, flat64 = heat.reshape(len(heat), -1), h64.reshape(len(h64), -1)
        safe = _top2_gap(flat64, 1) > ARGMAX_MARGIN
        assert safe.sum() >= 1
        assert np.array_equal(flat.argmax(1)[safe], flat64.argmax(1)[safe])
        c = N.first_flat_argmax(heat)
        assert np.array_equal(c, O.speedy_bargmax2d(torch.from_numpy(heat[:, 0])).numpy())
    # the two head orders are different sums: a restatement that ignored the order would not tell them apart
    assert not np.array_equal(heats["direct"], heats["w2p"])
    heat, corners = N.refinenet_exact(case.sd_rn, patches, deterministic)
    assert np.array_equal(heat, heats["direct" if deterministic else "w2p"])


def test_heat_restatement_ties_with_zero_head_weights(case):
    """convPb.weight = 0: every heat value is exactly the bias in both orders (the GPU tie tests rely on it)."""
    sd = dict(case.sd_rn)
    sd["convPb.weight"] = np.zeros_like(sd["convPb.weight"])
    patches = np.random.default_rng(5).uniform(-0.5, 0.5, (2, 24, 24)).astype(np.float32)
    body = N.refinenet_body(sd, patches, False)
    for order in ("direct", "w2p"):
        heat = N.refinenet_head(sd, body, order)
        assert np.all(heat == np.float32(sd["convPb.bias"][0]))
        assert np.array_equal(N.first_flat_argmax(heat), np.zeros((2, 2), np.int64))
