"""Host (no GPU) side of the trained-checkpoint regime (tests/trained_stats.py).

What the GPU tests (test_gpu_trained_stats.py) compare the kernels with is checked here against float64: the regime's own
assertions, the chained restatement on these weights, a float32 restatement of the fused tail's soft-max tree, and the per-layer
float64 bound.  The last section feeds the GPU tests' own assertion helpers deliberately wrong references; each must fail."""
import numpy as np
import pytest
import torch

import trained_stats as T
from oracle import deepcharuco_oracle as O
from oracle import net_exact as N
from oracle.conv_exact import conv_exact

# Restated fp32 chain against the float64 oracle graph in THIS regime (the sharpened heads multiply the logits' error by six, and
# the deterministic chain sums 1,152 terms in one sequence where Winograd sums 4 x 288).  Twice the largest gap measured on the
# test's own inputs; the restatement's summation orders are fixed, so a run repeats these to the last bit and the factor only
# covers other torch builds' float64 statistics.  Measured (frames 0 / 47 / 95 of the launch and the 67x101 frame; the 19
# restated patches, both head orders):   detector  default 5.27e-5   deterministic 9.87e-5   (torch fp32: 4.5e-5)
#                                          RefineNet default 2.08e-5   deterministic 2.94e-5   (torch fp32: 1.4e-5)
DET_F64_ATOL = {False: 1.06e-4, True: 1.98e-4}
HEAT_F64_ATOL = {False: 4.15e-5, True: 5.87e-5}
LAYER_K = T.LAYER_K

MODES = [False, True]
MODE_IDS = ["default", "deterministic"]


def _top2_gap(a, axis):
    s = np.sort(a, axis=axis)
    return np.take(s, -1, axis=axis) - np.take(s, -2, axis=axis)


# --------------------------------------------------------------------------- the regime itself

@pytest.mark.parametrize("kind", ["detector", "refinenet"])
def test_generator_puts_every_bn_layer_in_the_trained_regime(kind):
    from deepcharuco_amd import weights as W
    reg = T.detector_regime() if kind == "detector" else T.refinenet_regime()
    sd, info = reg["sd"], reg["info"]
    pooled = []
    for s in W.specs_for(kind):
        if s.bn is None:
            continue
        g, var, wt = sd[f"{s.bn}.weight"], sd[f"{s.bn}.running_var"], sd[f"{s.name}.weight"]
        live = var[var > 0]
        assert np.log10(live.max() / live.min()) >= 4.0 and (var == 0).sum() == 1 and (var >= 0).all(), s.name
        assert (g < 0).sum() >= 0.05 * len(g) and (g == 0).sum() == 1, s.name
        z = int(np.flatnonzero(var == 0)[0])
        assert not wt[z].any() and sd[f"{s.bn}.running_mean"][z] == sd[f"{s.name}.bias"][z], s.name
        norms = np.sqrt((wt.astype(np.float64) ** 2).sum((1, 2, 3)))
        assert np.log10(norms[norms > 0].max() / norms[norms > 0].min()) >= 2.5, s.name
        if s.pool:
            pooled.append(s.name)
            assert info[s.name]["pool_before_bn_share"] > 0 and info[s.name]["abs_gamma_share"] > 0, info[s.name]
    assert pooled == (["conv1b", "conv2b", "conv3b"] if kind == "detector" else ["conv2b"])
    # the same call gives the same weights: a numpy Generator and float64 reductions of one build
    again = T.trained_stats_state_dict(kind, T.DETECTOR_SEED if kind == "detector" else T.REFINENET_SEED,
                                       reg["images"][T.RESTATED] if kind == "detector" else reg["patches"][:16])[0]
    assert all(np.array_equal(again[k], sd[k]) for k in again if k.startswith("bn") or "conv" in k and kind == "refinenet")


def test_sharpened_heads_fire_and_span_the_probability_range():
    d = T.detector_regime()
    s = d["sharp"]
    assert len(s["firing_per_frame"]) == 96 and min(s["firing_per_frame"]) >= 8
    for key in ("p_loc_range", "p_ids_range"):
        assert s[key][0] < 0.5 and s[key][1] > 1 - 1e-5, s
    assert s["logit_range"][0] < -20 and s["logit_range"][1] > 20, s


# --------------------------------------------------------------------------- restatement against float64

@pytest.mark.parametrize("deterministic", MODES, ids=MODE_IDS)
def test_detector_restatement_vs_float64(deterministic):
    d = T.detector_regime()
    tol = DET_F64_ATOL[deterministic]
    worst = 0.0
    for which, images in (("batch", d["images"][T.RESTATED]), ("odd", N.normalised(d["odd"]))):
        l64, i64 = T.detector_logits64(d["sd"], images)
        loc, ids = T.restated_detector(deterministic, which)
        assert loc.dtype == np.float32 and loc.shape == l64.shape and ids.shape == i64.shape
        for got, ref in ((loc, l64), (ids, i64)):
            gap = float(np.abs(got - ref).max())
            worst = max(worst, gap)
            assert gap <= tol, (which, gap)
            safe = _top2_gap(ref, 1) > tol
            assert safe.sum() >= 0.9 * safe.size
            assert np.array_equal(got.argmax(1)[safe], ref.argmax(1)[safe])
    print(f"detector restatement vs float64, {'deterministic' if deterministic else 'default'}: {worst:.3g} (allowed {tol})")
    assert worst >= tol / 4, "the tolerance no longer describes this regime: measure again"
    # no -0.0 reaches the features: ReLU's sign of zero is not part of any comparison in this regime
    for f in T.restated_features(deterministic):
        assert not (np.signbit(f) & (f == 0)).any()
        assert 0.3 < (f == 0).mean() < 0.7                   # BN + ReLU outputs: about half exact zeros


@pytest.mark.parametrize("deterministic", MODES, ids=MODE_IDS)
def test_refinenet_restatement_vs_float64(deterministic):
    r = T.refinenet_regime()
    p = r["patches"][r["restated"]]
    h64 = O.refinenet_forward({k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in r["sd"].items()},
                              torch.from_numpy(p).double()[:, None]).numpy()
    heats = T.restated_heat(deterministic)
    tol = HEAT_F64_ATOL[deterministic]
    flat64 = h64.reshape(len(h64), -1)
    safe = _top2_gap(flat64, 1) > tol
    assert safe.sum() >= 0.9 * safe.size
    worst = 0.0
    for order in ("direct", "w2p"):
        heat = heats[order]
        assert heat.dtype == np.float32 and heat.shape == h64.shape
        gap = float(np.abs(heat - h64).max())
        worst = max(worst, gap)
        assert gap <= tol, (order, gap)
        assert np.array_equal(heat.reshape(len(heat), -1).argmax(1)[safe], flat64.argmax(1)[safe])
        assert np.array_equal(N.first_flat_argmax(heat), O.speedy_bargmax2d(torch.from_numpy(heat[:, 0])).numpy())
    print(f"RefineNet restatement vs float64, {'deterministic' if deterministic else 'default'}: {worst:.3g} (allowed {tol})")
    assert worst >= tol / 4, "the tolerance no longer describes this regime: measure again"
    assert not np.array_equal(heats["direct"], heats["w2p"])
    heat, corners = N.refinenet_exact(r["sd"], p[:2], deterministic)
    assert np.array_equal(heat, heats["direct" if deterministic else "w2p"][:2])


# --------------------------------------------------------------------------- the tail's confidence tree

def _cells(z):
    return np.moveaxis(z, 1, -1).reshape(-1, z.shape[1])


def test_confidence_tree_in_float32_stays_within_the_bound():
    """The float32 tree of dcx_tail.hip (16 couts per lane half ascending, halves re-based on the tile maximum, tiles on the
    overall maximum, 1 / sum) against the float64 soft-max, on every cell of the restated frames: loc (65 = two full tiles and
    one with a single valid row) and ids at n_ids + 1 = 17, 32, 33 and 64."""
    d = T.detector_regime()
    loc, ids = T.restated_detector(False)
    feats = T.restated_features(False)
    heads = {"loc65": loc, "ids17": ids}
    sharpest = 0.0
    for n_ids in (31, 32, 63):
        heads[f"ids{n_ids + 1}"] = N.detector_heads(T.widen_ids_head(d["sd"], 16, n_ids), feats)[1]
    for name, z in heads.items():
        zz = _cells(z)
        p = T.conf_tree_f32(zz)
        worst = T.assert_conf_within_bound(p, zz, name)
        units = float((np.abs(p - T.softmax_max64(zz)) / T.softmax_max64(zz) / T.U24).max())
        print(f"{name}: worst ratio to the bound {worst:.3f}, {units:.2f} units of 2^-24, smallest bound {T.conf_bound(zz).min() / T.U24:.1f}")
        assert worst <= 0.5                                   # the emulation has room: the GPU's expf may differ from numpy's
        # terms of this regime do vanish, and winners do come close to 1
        dmin = (zz.astype(np.float64) - zz.max(1, keepdims=True)).min()
        assert dmin < -30, (name, dmin)
        sharpest = max(sharpest, float(T.softmax_max64(zz).max()))
    assert sharpest > 1 - 1e-5, sharpest
    under = np.float32([[0.0] + [-120.0] * 32])               # every other term underflows, in both tiles: p == 1
    assert T.conf_tree_f32(under)[0] == 1.0
    T.assert_conf_within_bound(T.conf_tree_f32(under), under, "underflow")


def test_layer_restatement_within_half_the_float64_bound():
    """The K of the per-layer float64 check is twice what the restatement itself needs, per family, over TRAINED_BN_CASES."""
    worst = {}
    for name, n, cin, cout, h, w, pad, ups, pool, ks, has_bn in T.TRAINED_BN_CASES:
        x, wt, b, bn = T.trained_bn_layer(name, n, cin, cout, h, w, ks)
        assert 0.45 < (x == 0).mean() < 0.55 and x.min() == 0.0
        if not has_bn:
            ref, scale = T.layer_ref64(x, wt, b, None, pad, ups, pool)
            y = conv_exact(x, wt, b, None, pad=pad, family="direct")
            r = T.assert_layer_within_f64_bound(y, ref, scale, LAYER_K["direct"] / 2, f"{name} direct")
            print(f"{name}: raw head ratio {r:.2f}")
            continue
        g, _, mu, var = bn
        assert len({(float(a), float(c)) for a, c in zip(g, var)}) == 16 and np.abs(mu).max() > 25
        ref, scale = T.layer_ref64(x, wt, b, bn, pad, ups, pool)
        for fam in ["direct", "w2h"] + (["w2p"] if ups else []):
            y = conv_exact(x, wt, b, bn, pad=pad, ups=bool(ups), pool=bool(pool), family=fam)
            assert not (np.signbit(y) & (y == 0)).any()       # no -0.0: fmaxf's and v_max_f32's choice never shows
            r = T.assert_layer_within_f64_bound(y, ref, scale, LAYER_K[fam] / 2 * 1.001, f"{name} {fam}")
            worst[fam] = max(worst.get(fam, 0.0), r)
    print("worst ratio per family:", worst)
    assert all(worst[f] >= LAYER_K[f] / 4 for f in LAYER_K), worst


# --------------------------------------------------------------------------- reference mutants

POOLED_CASES = [c for c in T.TRAINED_BN_CASES if c[8]]


@pytest.mark.parametrize("mutant", ["pool_first", "abs_gamma"])
@pytest.mark.parametrize("case", POOLED_CASES, ids=[c[0] for c in POOLED_CASES])
def test_mutant_bn_references_fail_the_layer_assertions(case, mutant):
    """A pooled layer evaluated with pool before BN, or with |gamma|, must fail both assertions of the per-layer GPU test."""
    name, n, cin, cout, h, w, pad, ups, pool, ks, _ = case
    x, wt, b, bn = T.trained_bn_layer(name, n, cin, cout, h, w, ks)
    ref, scale = T.layer_ref64(x, wt, b, bn, pad, ups, pool)
    good = conv_exact(x, wt, b, bn, pad=pad, ups=bool(ups), pool=True, family="w2h")
    T.assert_same_bits(good, good.copy(), name)
    T.assert_layer_within_f64_bound(good, ref, scale, LAYER_K["w2h"], name)
    if mutant == "abs_gamma":
        bad = conv_exact(x, wt, b, [np.abs(bn[0])] + bn[1:], pad=pad, ups=bool(ups), pool=True, family="w2h")
    else:       # the raw accumulators pooled, BN + ReLU afterwards in the kernels' own fp32 expression
        raw = conv_exact(x, wt, np.zeros_like(b), None, pad=pad, ups=bool(ups), pool=True, family="direct")
        g, be, mu, var = [t.astype(np.float64) for t in bn]
        alpha = (g / np.sqrt(var + 1e-5)).astype(np.float32)
        beta2 = (be + (b - mu) * alpha.astype(np.float64)).astype(np.float32)
        bad = np.maximum(raw * alpha[None, :, None, None] + beta2[None, :, None, None], np.float32(0)).astype(np.float32)
    with pytest.raises(AssertionError, match="differ from the exact restatement"):
        T.assert_same_bits(bad, good, name)
    with pytest.raises(AssertionError, match="from float64"):
        T.assert_layer_within_f64_bound(bad, ref, scale, LAYER_K["w2h"], name)
    share = float((np.abs(bad - ref) > T.DISCRIMINATION_ATOL * np.maximum(1.0, np.abs(ref))).mean())
    print(f"{name} {mutant}: {share:.3f} of the outputs move")
    assert share > 0.01


@pytest.mark.parametrize("mutant", ["drop_tile", "pad_as_zero"])
def test_mutant_softmax_trees_fail_the_confidence_assertion(mutant):
    """A tree that drops one tile's partial sum, or counts the pad rows of the last tile as logit 0, must fail the bound."""
    loc, ids = T.restated_detector(False)
    d = T.detector_regime()
    wide = N.detector_heads(T.widen_ids_head(d["sd"], 16, 32), T.restated_features(False))[1]       # 33 rows: a second tile with one
    for name, z in (("loc65", loc), ("ids33", wide)):
        zz = _cells(z)
        T.assert_conf_within_bound(T.conf_tree_f32(zz), zz, name)
        bad = T.conf_tree_f32(zz, drop_tile=0) if mutant == "drop_tile" else T.conf_tree_f32(zz, pad_as_zero=True)
        with pytest.raises(AssertionError, match="x its bound"):
            T.assert_conf_within_bound(bad, zz, name)
