"""Weights in the regime of a trained checkpoint, and the comparison helpers of the tests that use them.

Every other weight set of the suite comes from ``weights.synthetic_state_dict``: BN gamma in (0.5, 1.5), running_var in (0.5, 1.5),
rows of one common scale, flat logits.  :func:`trained_stats_state_dict` moves the whole state dict where checkpoints live: conv
rows over 3.5 decades of scale, one dead row per layer (running_var exactly 0), running statistics that ARE the statistics of the
layer's output on the frames the test runs, gamma of both signs with one exact 0.  :func:`sharpen_heads` does the same for the two
1x1 heads: logits over tens of units, so that soft-max terms underflow and winning probabilities come within 1e-6 of 1.

The weights depend on float64 reductions (torch's summation order is the build's), so no SHA is pinned: tests write
``weights.state_dict_sha256`` of each run into the parity report instead.

The helpers at the end (:func:`assert_same_bits`, :func:`assert_layer_within_f64_bound`, :func:`assert_conf_within_bound`) are
the assertions of test_gpu_trained_stats.py; test_trained_stats_host.py feeds them deliberately wrong references (pool before BN,
|gamma|, a dropped soft-max tile, pad rows counted as logit 0) and checks that each of them fails."""
import numpy as np
import torch
import torch.nn.functional as F

from deepcharuco_amd import weights as W

ROW_SCALE = (1e-2, 30.0)       # log-uniform factor of every conv row (and its bias)
GAMMA_MEAN, GAMMA_STD = 0.6, 0.5
BETA_STD = 0.3
DISCRIMINATION_ATOL = 1e-3     # "much more than the fp32 noise": the chains' fp32 error is ~1e-5 on outputs of order 1
U24 = 2.0 ** -24


def _t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _bn_relu64(y, g, be, mu, var):
    return F.relu(F.batch_norm(y, _t64(mu), _t64(var), _t64(g), _t64(be), False, 0.0, W.BN_EPS))


def trained_stats_state_dict(kind, seed, calib, n_ids=16):
    """(state dict float32, info) -- ``synthetic_state_dict(kind, seed, n_ids)`` walked in forward order in float64 on ``calib``
    ((N, H, W) normalised frames, or (K, 24, 24) patches for "refinenet").  Per BN layer: every conv row and its bias times a
    log-uniform factor in ROW_SCALE; one row zeroed (its output is its bias: mean = bias, variance exactly 0); running_mean /
    running_var = the float64 statistics of the conv's output on ``calib`` (population variance), rounded to float32; gamma ~
    N(0.6, 0.5) with one exact 0; beta ~ N(0, 0.3).  The 1x1 heads stay as drawn.

    info[layer] = dict(var_decades, negative_gammas, zero_row, zero_gamma) and, for pooled layers, ``pool_before_bn_share`` /
    ``abs_gamma_share``: the share of that layer's float64 outputs on ``calib`` that a pool-before-BN evaluation / one with
    |gamma| changes by more than DISCRIMINATION_ATOL.  The assertions of the regime are made here."""
    rng = np.random.default_rng([seed, 0 if kind == "detector" else 1, 20240])
    sd = {k: v.copy() for k, v in W.synthetic_state_dict(kind, seed, n_ids).items()}
    x = _t64(calib).reshape((-1, 1) + tuple(np.shape(calib)[-2:]))
    info = {}
    branch = None                # the detector's two head branches read the same conv4b output
    for s in W.specs_for(kind, n_ids):
        if s.bn is None:
            continue
        if kind == "detector" and s.name in ("convPa", "convDa"):
            branch = x if branch is None else branch
            x = branch
        c = s.cout
        f = np.exp(rng.uniform(np.log(ROW_SCALE[0]), np.log(ROW_SCALE[1]), c)).astype(np.float32)
        wt = (sd[f"{s.name}.weight"] * f[:, None, None, None]).astype(np.float32)
        b = (sd[f"{s.name}.bias"] * f).astype(np.float32)
        zero_row, zero_gamma = [int(v) for v in rng.choice(c, 2, replace=False)]
        wt[zero_row] = 0.0
        y = F.conv2d(x, _t64(wt), _t64(b), padding=s.pad)
        mu = y.mean((0, 2, 3)).numpy()
        var = y.var((0, 2, 3), unbiased=False).numpy()
        mu[zero_row], var[zero_row] = float(b[zero_row]), 0.0       # exactly, whatever the reduction rounds to
        g = rng.normal(GAMMA_MEAN, GAMMA_STD, c).astype(np.float32)
        g[zero_gamma] = 0.0
        be = rng.normal(0.0, BETA_STD, c).astype(np.float32)
        mu, var = mu.astype(np.float32), var.astype(np.float32)
        sd[f"{s.name}.weight"], sd[f"{s.name}.bias"] = wt, b
        sd[f"{s.bn}.weight"], sd[f"{s.bn}.bias"] = g, be
        sd[f"{s.bn}.running_mean"], sd[f"{s.bn}.running_var"] = mu, var

        live = var[var > 0]
        decades = float(np.log10(live.max() / live.min()))
        neg = int((g < 0).sum())
        assert decades >= 4.0 and int((var == 0).sum()) == 1, (kind, s.name, decades)
        assert neg >= 0.05 * c and int((g == 0).sum()) == 1, (kind, s.name, neg, c)
        info[s.name] = dict(var_decades=decades, negative_gammas=neg, zero_row=zero_row, zero_gamma=zero_gamma)

        out = _bn_relu64(y, g, be, mu, var)
        if s.pool:
            good = F.max_pool2d(out, 2, 2)
            pool_first = _bn_relu64(F.max_pool2d(y, 2, 2), g, be, mu, var)
            abs_gamma = F.max_pool2d(_bn_relu64(y, np.abs(g), be, mu, var), 2, 2)
            for key, bad in (("pool_before_bn_share", pool_first), ("abs_gamma_share", abs_gamma)):
                share = float(((bad - good).abs() > DISCRIMINATION_ATOL).double().mean())
                assert share > 0, (kind, s.name, key)
                info[s.name][key] = share
            out = good
        if s.ups:
            out = F.interpolate(out, scale_factor=2, mode="nearest")
        x = out
    W.validate_state_dict(sd, kind, n_ids)
    return sd, info


def detector_logits64(sd, images):
    """The oracle graph in float64 on float32 weights: images (N, H, W) normalised -> (loc, ids) float64 numpy."""
    from oracle import deepcharuco_oracle as O
    t = {k: _t64(v) for k, v in sd.items()}
    loc, ids = O.detector_forward(t, _t64(images)[:, None])
    return loc.numpy(), ids.numpy()


def _heads64(sd, feats):
    """The two raw 1x1 heads (net.py:74,77) in float64 on float64 features (convPa, convDa outputs)."""
    with torch.no_grad():
        return tuple(F.conv2d(f, _t64(sd[f"{c}.weight"]), _t64(sd[f"{c}.bias"])).numpy() for f, c in zip(feats, ("convPb", "convDb")))


def _features64(sd, images):
    """Everything below the heads in float64, by hooking the oracle graph's own two head convolutions."""
    from oracle import deepcharuco_oracle as O
    t = {k: _t64(v) for k, v in sd.items()}
    for c in ("convPb", "convDb"):          # identity heads: x * 1 + zeros is exact, so the "logits" are the features
        t[f"{c}.weight"] = torch.eye(256, dtype=torch.float64).view(256, 256, 1, 1)
        t[f"{c}.bias"] = torch.zeros(256, dtype=torch.float64)
    return O.detector_forward(t, _t64(images)[:, None])


def softmax_max64(z, axis=1):
    """Float64 soft-max probability of the arg-max class: 1 / sum exp(z - max)."""
    z = np.asarray(z, np.float64)
    return 1.0 / np.exp(z - z.max(axis=axis, keepdims=True)).sum(axis=axis)


def firing(loc, ids, dust_bin):
    """pred_argmax's rule (model_utils.py:53-78) on (N, C, h, w) logits: the boolean map of the cells that fire."""
    la, ia = loc.argmax(1), ids.argmax(1)
    return (la != 64) & (ia != dust_bin)


def sharpen_heads(sd, images, n_ids=16, scale=6.0, per_frame=10, frac=(0.55, 0.8)):
    """(state dict, info): convPb / convDb weights times ``scale``, then the no-corner bias shifted
    (weights.loc_nocorner_bias_shift) and the dust-bin bias calibrated to ~``per_frame`` firing cells per frame, both on the
    float64 oracle's logits of ``images`` ((N, H, W) normalised), as test_gpu_parity._masked_regime does.  ``frac`` is the share of
    cells class 64 takes: lower than a 240x320 frame's 85-95 %, because a 64x96 frame has 96 cells and eight of them must fire.
    Asserts >= 8 firing cells per frame, and that the float64 p_loc and p_ids of the firing cells reach below 0.5 and above
    1 - 1e-5."""
    sd = {k: v.copy() for k, v in sd.items()}
    for conv in ("convPb", "convDb"):
        sd[f"{conv}.weight"] = (sd[f"{conv}.weight"] * np.float32(scale)).astype(np.float32)
    feats = _features64(sd, images)
    loc, ids = _heads64(sd, feats)
    sd["convPb.bias"][64] = np.float32(sd["convPb.bias"][64] + np.float32(W.loc_nocorner_bias_shift(loc, *frac)))
    loc, ids = _heads64(sd, feats)
    m = ids[:, :n_ids].max(1) - ids[:, n_ids]
    m = -np.sort(-np.where(loc.argmax(1) == 64, -1e30, m).reshape(len(m), -1), axis=1)
    t = (m[:, per_frame - 1] + m[:, per_frame]) / 2
    assert (m[:, per_frame] > -1e29).all(), "a frame has too few unmasked cells"
    sd["convDb.bias"][n_ids] = np.float32(sd["convDb.bias"][n_ids] + np.float32(t.min()))
    loc, ids = _heads64(sd, feats)
    fire = firing(loc, ids, n_ids)
    per = fire.reshape(len(fire), -1).sum(1)
    assert per.min() >= 8, per
    p_loc, p_ids = softmax_max64(loc)[fire], softmax_max64(ids)[fire]
    for p in (p_loc, p_ids):
        assert p.min() < 0.5 and p.max() > 1 - 1e-5, (p.min(), p.max())
    best = np.where(fire, np.maximum(softmax_max64(loc), softmax_max64(ids)), 0.0).reshape(len(fire), -1).max(1)
    info = dict(firing_per_frame=per.tolist(), sharpest_frame=int(best.argmax()), logit_range=[float(min(loc.min(), ids.min())), float(max(loc.max(), ids.max()))],
                p_loc_range=[float(p_loc.min()), float(p_loc.max())], p_ids_range=[float(p_ids.min()), float(p_ids.max())],
                loc64_frac=float((loc.argmax(1) == 64).mean()))
    return sd, info


# --------------------------------------------------------------------------- the fused tail's confidence tree, restated

def conf_tree_f32(z, drop_tile=None, pad_as_zero=False):
    """Float32 restatement of dcx_tail.hip's soft-max (CONF): z (cells, C) float32 logits of ONE head -> (cells,) float32
    probability of the arg-max class.  Tiles of 32 couts; in a tile lane half h holds couts m0 + 8 q + 4 h + r (q, r = 0..3),
    summed in ascending order from 0 relative to the half's own maximum; the halves re-based on the tile's maximum, half 0 first;
    the tiles re-based on the overall maximum, ascending; 1 / sum.  Couts >= C (pad rows) take no part.
    drop_tile / pad_as_zero build the deliberately wrong trees of the reference-mutant tests."""
    z = np.ascontiguousarray(z, np.float32)
    n, c = z.shape
    f32 = np.float32
    tiles = []
    with np.errstate(under="ignore", invalid="ignore"):
        for m0 in range(0, c, 32):
            halves = []
            for h in (0, 1):
                cols = [m0 + 8 * q + 4 * h + r for q in range(4) for r in range(4)]
                if pad_as_zero:
                    v = np.stack([z[:, co] if co < c else np.zeros(n, f32) for co in cols], 1)
                else:
                    v = np.stack([z[:, co] for co in cols if co < c], 1) if cols[0] < c else np.zeros((n, 0), f32)
                if v.shape[1] == 0:
                    halves.append(None)
                    continue
                best = v.max(1)
                s = np.zeros(n, f32)
                for k in range(v.shape[1]):
                    s = (s + np.exp((v[:, k] - best).astype(f32)).astype(f32)).astype(f32)
                halves.append((best, s))
            best = halves[0][0] if halves[1] is None else np.maximum(halves[0][0], halves[1][0])
            a = (halves[0][1] * np.exp((halves[0][0] - best).astype(f32)).astype(f32)).astype(f32)
            cc = np.zeros(n, f32) if halves[1] is None else (halves[1][1] * np.exp((halves[1][0] - best).astype(f32)).astype(f32)).astype(f32)
            tiles.append((best, (a + cc).astype(f32)))
        top = np.max(np.stack([t[0] for t in tiles]), 0)
        s = np.zeros(n, f32)
        for i, (best, part) in enumerate(tiles):
            if i == drop_tile:
                continue
            s = (s + (part * np.exp((best - top).astype(f32)).astype(f32)).astype(f32)).astype(f32)
        return (f32(1.0) / s).astype(f32)


# Relative error of one confidence in units of 2^-24, counted on dcx_tail.hip (the library is built without fast-math: expf is
# ocml's, 1 ulp = 2 units; the division is correctly rounded, 1 unit):
#   a term passes   expf(logit - half max)        2      the subtraction's rounding is the first term of the bound, see below
#                   the half's 16-term sum        15     additions of positive terms, 1 unit each on the running sum
#                   * expf(half max - tile max)   2 + 1
#                   half 0 + half 1               1
#                   * expf(tile max - max)        2 + 1
#                   the tiles' sum                2      (three loc tiles / two ids tiles; the first addition is to 0)
#                   1 / sum                       1      -> 27 units, 18 additions among them; the bound allows 32
# Each of the three subtractions rounds by at most 2^-24 of its own size, which is at most |d_c| = |logit_c - max|, and moves the
# term by that relative amount: 3 |d_c| per term, weighted by the term's share of the sum.  A term that underflows is smaller
# than 2^-126 against a sum >= 1.
CONF_BOUND_CONST = 32.0


def conf_bound(z, axis=1):
    """Per-cell bound on the relative error of the tail's confidence: 2^-24 (3 sum |d_c| e^d_c / sum e^d_c + 32), in float64."""
    z = np.asarray(z, np.float64)
    d = z - z.max(axis=axis, keepdims=True)
    e = np.exp(d)
    return U24 * (3.0 * (np.abs(d) * e).sum(axis=axis) / e.sum(axis=axis) + CONF_BOUND_CONST)


def assert_conf_within_bound(got, z, what, axis=1):
    """got: float32 confidences, z: the logits the kernel holds (its very bits, restated).  Returns the worst ratio to the bound."""
    exp = softmax_max64(z, axis)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == exp.shape, (what, got.dtype, got.shape, exp.shape)
    ratio = np.abs(got.astype(np.float64) - exp) / exp / conf_bound(z, axis)
    worst = float(ratio.max()) if ratio.size else 0.0
    assert np.isfinite(ratio).all() and worst <= 1.0, f"{what}: confidence off by {worst:.3g} x its bound"
    return worst


# --------------------------------------------------------------------------- per-layer comparisons

def assert_same_bits(got, exp, what):
    """Equality of every bit, the sign of zero included."""
    got, exp = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(exp, np.float32)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} output elements were never written"
    bad = got.view(np.uint32) != exp.view(np.uint32)
    zero_sign = int((bad & (got == 0) & (exp == 0)).sum())
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {got.size} elements differ from the exact restatement "
                           f"({zero_sign} of them in the sign of zero only; max abs {np.abs(got - exp)[bad].max()})")


def layer_ref64(x, wt, b, bn, pad, ups, pool, abs_gamma=False, pool_first=False):
    """(float64 output, element-wise error scale) of conv + BN + ReLU [+ pool] on float32 data.  The scale is
    |alpha| sum |w x| + |beta2| with alpha = gamma / sqrt(var + eps), beta2 = beta + (bias - mean) alpha, all float64; pooled
    with the output (max is 1-Lipschitz, so the largest scale of a window bounds the window's maximum).
    abs_gamma / pool_first: the deliberately wrong references of the reference-mutant tests."""
    x, wt, b = _t64(x), _t64(wt), _t64(b)
    if bn is None:                                   # raw 1x1 heads: acc + bias, scale sum |w x| + |bias|
        assert not (ups or pool)
        sh = (1, -1, 1, 1)
        return (F.conv2d(x, wt, b, padding=pad).numpy(), (F.conv2d(x.abs(), wt.abs(), None, padding=pad) + b.abs().view(sh)).numpy())
    g, be, mu, var = [_t64(t) for t in bn]
    if abs_gamma:
        g = g.abs()
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    acc = F.conv2d(x, wt, None, padding=pad)
    mag = F.conv2d(x.abs(), wt.abs(), None, padding=pad)
    alpha = g / torch.sqrt(var + W.BN_EPS)
    beta2 = be + (b - mu) * alpha
    sh = (1, -1, 1, 1)
    scale = alpha.abs().view(sh) * mag + beta2.abs().view(sh)
    if pool and pool_first:
        acc = F.max_pool2d(acc, 2, 2)
    y = F.relu(acc * alpha.view(sh) + beta2.view(sh))
    if pool:
        y = y if pool_first else F.max_pool2d(y, 2, 2)
        scale = F.max_pool2d(scale, 2, 2)
    return y.numpy(), scale.numpy()


# The K of assert_layer_within_f64_bound per kernel family, in units of 2^-24 (|alpha| sum |w x| + |beta2|): twice the exact
# restatement's own worst ratio over TRAINED_BN_CASES, measured on the CPU (test_trained_stats_host.py repeats the measurement):
# direct 6.27 (T_ups_partial_10x12), w2h 4.17 (T_heads512_8x12), w2p 4.97 (T_ups_partial_10x12).
LAYER_K = {"direct": 12.6, "w2h": 8.4, "w2p": 10.0}


def layer_f64_ratio(got, ref64, scale):
    """Largest |got - float64| in units of 2^-24 x the element's scale."""
    err = np.abs(np.asarray(got, np.float64) - ref64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / (U24 * scale))
    return float(r.max())


def assert_layer_within_f64_bound(got, ref64, scale, k, what):
    worst = layer_f64_ratio(got, ref64, scale)
    assert np.isfinite(worst) and worst <= k, f"{what}: {worst:.3g} x 2^-24 x scale from float64, allowed {k}"
    return worst


def trained_bn_layer(name, n, cin, cout, h, w, ks, seed_offset=0):
    """Input, weights and BN of one TRAINED_BN_CASES layer (numpy float32).  Input: ReLU-like -- half exact zeros, non-negative,
    per-channel scales over three decades.  BN per channel from gamma in {-1.3, -1e-3, 0, 0.7} x var in {0, 1e-7, 1e-3, 50},
    every pair present (16 pairs, cout >= 64), mean up to +-30, beta ~ N(0, 0.3)."""
    import zlib
    rng = np.random.default_rng([zlib.crc32(name.encode()), seed_offset])
    scale = np.exp(rng.uniform(np.log(1e-2), np.log(10.0), cin))
    x = np.abs(rng.standard_normal((n, cin, h, w))) * scale[None, :, None, None]
    x[rng.random(x.shape) < 0.5] = 0.0
    wt = rng.standard_normal((cout, cin, ks, ks)) * np.sqrt(2.0 / (cin * ks * ks))
    b = rng.standard_normal(cout) * 0.1
    gammas, variances = np.float32([-1.3, -1e-3, 0.0, 0.7]), np.float32([0.0, 1e-7, 1e-3, 50.0])
    pair = rng.permutation(np.arange(cout) % 16)
    assert cout >= 16 and len(set(pair.tolist())) == 16
    g, var = gammas[pair % 4], variances[pair // 4]
    mu = rng.uniform(-30.0, 30.0, cout)
    be = rng.standard_normal(cout) * 0.3
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return f(x), f(wt), f(b), [f(g), f(be), f(mu), f(var)]


# (name, n, cin, cout, h, w, pad, ups, pool, ks, bn): the smallest shapes that between them, under DCX_FORCE_CFG, reach every
# convolution instantiation but the fused RefineNet heads (partial tiles, odd pooled maps, valid padding, up-sampled reads with
# one and two cout tiles, the grouped 8x8 / 6x6 maps with an odd image count, the 512-channel head layer, the raw 1x1)
TRAINED_BN_CASES = [
    ("T_partial_13x45", 1, 64, 64, 13, 45, 1, 0, 0, 3, True),
    ("T_pool_odd_25x37", 2, 64, 64, 25, 37, 1, 0, 1, 3, True),
    ("T_valid_pool_odd_23x21", 3, 128, 128, 23, 21, 0, 0, 1, 3, True),
    ("T_valid_20x20_64to128", 3, 64, 128, 20, 20, 0, 0, 0, 3, True),
    ("T_ups_8x8_128to128", 3, 128, 128, 8, 8, 1, 1, 0, 3, True),
    ("T_ups_partial_10x12", 2, 64, 64, 10, 12, 1, 1, 0, 3, True),
    ("T_grouped_8x8_odd_count", 5, 128, 128, 8, 8, 1, 0, 0, 3, True),
    ("T_grouped_6x6", 3, 64, 64, 6, 6, 1, 0, 0, 3, True),
    ("T_heads512_8x12", 1, 128, 512, 8, 12, 1, 0, 0, 3, True),
    ("T_k1_raw_17", 2, 256, 17, 6, 9, 0, 0, 0, 1, False),
]


# --------------------------------------------------------------------------- the inputs both test files run

DETECTOR_SEED, REFINENET_SEED = 7008, 7101      # seeds whose draws pass the generator's and sharpen_heads' assertions
RESTATED = [0, 47, 95]                           # frames of the 96-frame launch that are restated (two boards, one noise frame)
K_RUNS = {1: [0], 16: list(range(16)), 113: [0, 57, 100, 112]}     # RefineNet launches and the patches restated in each
_REGIME = {}


def detector_regime():
    """96 frames of 64x96 (48 boards, 48 noise), one 67x101 board, and detector weights in the trained regime: BN statistics
    calibrated on the RESTATED frames, heads sharpened on all 96."""
    if "detector" not in _REGIME:
        from oracle import net_exact as N
        frames = np.concatenate([W.synthetic_frames("board", 5101, 48, 64, 96), W.synthetic_frames("noise", 5102, 48, 64, 96)])
        odd = W.synthetic_frames("board", 5103, 1, 67, 101)
        images = N.normalised(frames)
        sd, info = trained_stats_state_dict("detector", DETECTOR_SEED, images[RESTATED])
        sd, sharp = sharpen_heads(sd, images)
        _REGIME["detector"] = dict(frames=frames, odd=odd, images=images, sd=sd, info=info, sharp=sharp, n_ids=16,
                                   sha=W.state_dict_sha256(sd, "detector", 16))
    return _REGIME["detector"]


def refinenet_regime():
    """113 patches of the detector regime's first frame around key-points all over it, the four frame corners first, and
    RefineNet weights whose BN statistics are those of the first 16 patches."""
    if "refinenet" not in _REGIME:
        from oracle import deepcharuco_oracle as O
        d = detector_regime()
        rng = np.random.default_rng(77)
        h, w = d["frames"].shape[1:]
        kp = np.stack([rng.integers(0, w, 113), rng.integers(0, h, 113)], 1)
        kp[:4] = [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]]
        patches = O.extract_patches(torch.from_numpy(d["images"][0][None]), torch.from_numpy(kp)).numpy()
        sd, info = trained_stats_state_dict("refinenet", REFINENET_SEED, patches[:16])
        _REGIME["refinenet"] = dict(patches=patches, kp=kp, sd=sd, info=info, sha=W.state_dict_sha256(sd, "refinenet"),
                                    restated=sorted({i for v in K_RUNS.values() for i in v}))
    return _REGIME["refinenet"]


def restated_detector(mode, which="batch"):
    """detector_exact on the RESTATED frames ("batch"), the 67x101 frame ("odd") or a tuple of frame indices, in one mode,
    computed once."""
    key = ("restated", bool(mode), which)
    if key not in _REGIME:
        from oracle import net_exact as N
        d = detector_regime()
        frames = d["frames"][RESTATED] if which == "batch" else d["odd"] if which == "odd" else d["frames"][list(which)]
        _REGIME[key] = N.detector_exact(d["sd"], frames, deterministic=bool(mode))
    return _REGIME[key]


def restated_features(mode):
    """detector_features (convPa, convDa outputs) of the RESTATED frames in one mode, computed once."""
    key = ("features", bool(mode))
    if key not in _REGIME:
        from oracle import net_exact as N
        d = detector_regime()
        _REGIME[key] = N.detector_features(d["sd"], d["images"][RESTATED], bool(mode))
    return _REGIME[key]


def restated_heat(mode):
    """{head order: heat (len(restated), 1, 64, 64)} of the refinenet regime's restated patches in one mode, computed once."""
    key = ("heat", bool(mode))
    if key not in _REGIME:
        from oracle import net_exact as N
        r = refinenet_regime()
        body = N.refinenet_body(r["sd"], r["patches"][r["restated"]], bool(mode))
        _REGIME[key] = {o: N.refinenet_head(r["sd"], body, o) for o in ("direct", "w2p")}
    return _REGIME[key]


def widen_ids_head(sd, n_ids, new_n_ids, seed=0):
    """More ids rows over the same backbone, the dust bin staying last (as test_gpu_exact_chain.test_fused_tail_ties adds
    them): rows and biases drawn at the spread of the existing ones."""
    sd = {k: v.copy() for k, v in sd.items()}
    rng = np.random.default_rng([new_n_ids, seed])
    w0, b0 = sd["convDb.weight"], sd["convDb.bias"]
    assert w0.shape[0] == n_ids + 1 and new_n_ids > n_ids
    extra = (rng.standard_normal((new_n_ids - n_ids,) + w0.shape[1:]) * w0[:-1].std()).astype(np.float32)
    sd["convDb.weight"] = np.concatenate([w0[:-1], extra, w0[-1:]])
    sd["convDb.bias"] = np.concatenate([b0[:-1], (rng.standard_normal(len(extra)) * b0[:-1].std()).astype(np.float32), b0[-1:]])
    return sd


def expected_corners(loc1, ids1, dust_bin):
    """One frame's firing cells from ITS logits (1, C, hc, wc), in infer_batch's order (by id, stable over raster order):
    (rows (K, 3) int64 [x, y, id], loc logits (K, 65), ids logits (K, n_ids + 1)) -- the logits behind every confidence."""
    la, ia = loc1[0].argmax(0), ids1[0].argmax(0)
    fire = (la != 64) & (ia != dust_bin)
    cy, cx = np.nonzero(fire)
    order = np.argsort(ia[cy, cx], kind="stable")
    cy, cx = cy[order], cx[order]
    l = la[cy, cx]
    rows = np.stack([8 * cx + l % 8, 8 * cy + l // 8, ia[cy, cx]], 1).astype(np.int64)
    return rows, loc1[0][:, cy, cx].T, ids1[0][:, cy, cx].T
