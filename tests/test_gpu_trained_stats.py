"""Every kernel family on weights in the regime of a trained checkpoint (tests/trained_stats.py), bit for bit against the exact
restatement, and the fused tail's confidences against the float64 soft-max of the restated logits.

What no other weight set of the suite has: BN gamma of both signs and exactly 0 (a positive slope commutes with the max-pool: a
kernel that pooled before BN, or took |alpha|, passes everything else), running_var over seven decades and exactly 0 (alpha =
316 gamma, a cancelling beta2), running statistics that are the layer's own, ReLU-like inputs, conv rows over 3.5 decades, and
heads sharp enough that soft-max terms underflow and probabilities come within 1e-6 of 1.  test_trained_stats_host.py holds the
restatement to float64 in this regime and shows that the assertions used here fail on wrong references."""
import os

import numpy as np
import pytest
import torch

import trained_stats as T
from deepcharuco_amd import weights as W
from oracle import deepcharuco_oracle as O
from oracle import net_exact as N
from oracle.conv_exact import conv_exact
from test_gpu_exact_chain import HEAT_CFGS, _frame_rows, _rows_equal
from test_gpu_parity import _conv_layer, _family, _report

pytestmark = pytest.mark.gpu

MODES = [False, True]
MODE_IDS = ["default", "deterministic"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture
def mode(request):
    """set_deterministic(param) for the test, default mode afterwards; DCX_FORCE_CFG is never inherited."""
    from deepcharuco_amd.inference import set_deterministic
    os.environ.pop("DCX_FORCE_CFG", None)
    set_deterministic(request.param)
    yield request.param
    set_deterministic(False)


def _mode_id(mode):
    return MODE_IDS[int(mode)]


# --------------------------------------------------------------------------- 1. one layer at a time

def _run_layer(dev, case, data):
    name, n, cin, cout, h, w, pad, ups, pool, ks, has_bn = case
    x, wt, b, bn = data
    t = torch.from_numpy
    return _conv_layer(t(x).to(dev), t(wt), t(b), [t(a) for a in bn] if has_bn else None, pad, ups, pool, ks).cpu().numpy()


def _pick(case):
    from deepcharuco_amd import _lib
    name, n, cin, cout, h, w, pad, ups, pool, ks, has_bn = case
    ho, wo = (h << ups) + 2 * pad - (ks - 1), (w << ups) + 2 * pad - (ks - 1)
    return _lib.lib().dcx_conv_pick_name_ups(n, cin, ho, wo, cout, ks, int(pool), 0 if has_bn else 1, int(ups)).decode()


def _exact(case, data, fam):
    name, n, cin, cout, h, w, pad, ups, pool, ks, has_bn = case
    x, wt, b, bn = data
    return conv_exact(x, wt, b, bn if has_bn else None, pad=pad, ups=bool(ups), pool=bool(pool), family=fam)


@pytest.mark.parametrize("case", T.TRAINED_BN_CASES, ids=[c[0] for c in T.TRAINED_BN_CASES])
def test_trained_bn_layer_under_the_family_rule(dev, case):
    """The instantiation the family rule picks, on a ReLU-like input with BN drawn from gamma in {-1.3, -1e-3, 0, 0.7} x var in
    {0, 1e-7, 1e-3, 50} and |mean| up to 30: every bit of the restatement of that family (the output is NaN-prefilled, so an
    unwritten element shows; the sign of zero is compared as it is -- the restatement holds no -0.0 on these inputs, see
    test_trained_stats_host.py, so fmaxf's and v_max_f32's choice for max(-0, +0) cannot hide a difference), and float64 torch
    within K 2^-24 (|alpha| sum |w x| + |beta2|) per element."""
    name, n, cin, cout, h, w, pad, ups, pool, ks, has_bn = case
    os.environ.pop("DCX_FORCE_CFG", None)
    data = T.trained_bn_layer(name, n, cin, cout, h, w, ks)
    got = _run_layer(dev, case, data)
    picked = _pick(case)
    fam = _family(picked)
    T.assert_same_bits(got, _exact(case, data, fam), f"{name} [{picked}]")
    ref64, scale = T.layer_ref64(data[0], data[1], data[2], data[3] if has_bn else None, pad, ups, pool)
    ratio = T.assert_layer_within_f64_bound(got, ref64, scale, T.LAYER_K[fam], name)
    _report(f"trained_stats/layer/{name}", dict(kernel=picked[picked.find("dcx_conv_") + 9:], family=fam, differing_bits=0,
                                                 f64_ratio=ratio, f64_ratio_allowed=T.LAYER_K[fam],
                                                 negative_zeros=int((np.signbit(got) & (got == 0)).sum())))


def test_trained_bn_every_conv_instantiation_bit_exact(dev, monkeypatch):
    """DCX_FORCE_CFG walks every instantiation dcx_profile_kernel_name lists (the fused RefineNet heads have their own test
    below) over every TRAINED_BN_CASES shape it can run: all of them must give the bits of their family's restatement, and none
    may be left out -- the pooled epilogues (direct quad-max, direct in-lane, wino2h, wino2h small, wino2hs) among them."""
    from deepcharuco_amd import _lib
    L = _lib.lib()
    names = []
    while True:
        nm = L.dcx_profile_kernel_name(len(names)).decode()
        if nm == "?":
            break
        names.append(nm)
    assert len(names) >= 14 and sum("wino2h" in n_ for n_ in names) >= 5
    ran, pooled = {}, set()
    for case in T.TRAINED_BN_CASES:
        name, n, cin, cout, h, w, pad, ups, pool, ks, has_bn = case
        data = T.trained_bn_layer(name, n, cin, cout, h, w, ks, seed_offset=1)
        refs = {}
        for cfg in names:
            if "HEAT" in cfg:
                continue
            monkeypatch.setenv("DCX_FORCE_CFG", cfg)
            if _pick(case) != cfg:
                continue      # this instantiation cannot run this layer (kernel size / pooling / cout tile / up-sampling)
            got = _run_layer(dev, case, data)
            fam = _family(cfg)
            if fam not in refs:
                refs[fam] = _exact(case, data, fam)
            T.assert_same_bits(got, refs[fam], f"{cfg} on {name}")
            ran[cfg] = ran.get(cfg, 0) + 1
            if pool:
                pooled.add(cfg)
    monkeypatch.delenv("DCX_FORCE_CFG")
    _report("trained_stats/conv_instantiations_bitexact", dict(ran=ran, pooled=sorted(pooled), differing_bits=0))
    missing = [c for c in names if "HEAT" not in c and c not in ran]
    assert not missing, f"instantiations never exercised: {missing}"
    assert len(pooled) >= 5, pooled


# --------------------------------------------------------------------------- 2. detector logits

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS, indirect=True)
def test_detector_logits_bit_exact_on_trained_stats(dev, mode):
    """forward_u8 and forward == detector_exact, every logit: B = 1 at 64x96 and 67x101, B = 3, and a 96-frame launch with frames
    0 / 47 / 95 restated.  Every launch runs the family the restatement assumes."""
    from deepcharuco_amd import _lib
    from deepcharuco_amd.models.net import dcModel
    L = _lib.lib()
    d = T.detector_regime()
    dc = dcModel(16, d["sd"], dev)
    batch, odd = T.restated_detector(mode), T.restated_detector(mode, "odd")
    runs = [("B1", d["frames"][:1], [0], [e[:1] for e in batch]), ("B1_67x101", d["odd"], [0], odd),
            ("B3", d["frames"][T.RESTATED], [0, 1, 2], batch), ("B96", d["frames"], T.RESTATED, batch)]
    for tag, frames, sel, (loc, ids) in runs:
        n, h, w = frames.shape
        for name, fam, args in N.detector_layers(n, h, w, 16, mode):
            picked = L.dcx_conv_pick_name_ups(*args).decode()
            assert _family(picked) == fam, (name, tag, picked, fam)
        out = dc.forward_u8(torch.from_numpy(frames).to(dev))
        out_f = dc.forward(torch.from_numpy(N.normalised(frames)[:, None]).to(dev))
        for key, exp in (("loc", loc), ("ids", ids)):
            for kind, o in (("u8", out), ("f32", out_f)):
                T.assert_same_bits(o[key].cpu().numpy()[sel], exp, f"{key} ({kind}) {tag} {_mode_id(mode)}")
    _report(f"trained_stats/detector/{_mode_id(mode)}", dict(differing_bits=0, launches=[r[0] for r in runs], weights_sha256=d["sha"],
                                                             bn_layers=d["info"], heads=d["sharp"]))


# --------------------------------------------------------------------------- 3. RefineNet heat

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS, indirect=True)
def test_refinenet_heat_bit_exact_on_trained_stats(dev, mode, monkeypatch):
    """RefineNet.forward == refinenet_exact at K = 1, 16, 113 (patches of the four frame corners first), under the family rule
    and with each HEAT instantiation forced; infer_patches' corners and xy == the restated first flat arg-max."""
    from deepcharuco_amd.models.refinenet import RefineNet
    r = T.refinenet_regime()
    rn = RefineNet(r["sd"], dev)
    exp = T.restated_heat(mode)
    natural = N.family_of(64, 64, 3, 0, "heat", 1, mode)
    pos = {i: j for j, i in enumerate(r["restated"])}
    pool, kp = r["patches"], r["kp"]
    for head in (None, "direct", "w2p"):
        if head is None:
            monkeypatch.delenv("DCX_FORCE_CFG", raising=False)
        else:
            monkeypatch.setenv("DCX_FORCE_CFG", HEAT_CFGS[head])
        order = head or natural
        for k, idx in T.K_RUNS.items():
            p = torch.from_numpy(pool[:k]).to(dev)
            heat = rn(p[:, None]).cpu().numpy()
            e = exp[order][[pos[i] for i in idx]]
            T.assert_same_bits(heat[idx], e, f"heat K={k}, head {order}, {_mode_id(mode)}")
            cog, c = rn.infer_patches(p, torch.from_numpy(kp[:k]).to(dev))
            ec = N.first_flat_argmax(e)
            assert np.array_equal(c.cpu().numpy()[idx], ec), f"K={k}, head {order}: corners"
            exy = ((torch.from_numpy(ec) - 32) / 8 + torch.from_numpy(kp[idx])).numpy()
            assert np.array_equal(cog.cpu().numpy()[idx], exy)
    monkeypatch.delenv("DCX_FORCE_CFG", raising=False)
    _report(f"trained_stats/refinenet/{_mode_id(mode)}", dict(differing_bits=0, k_runs=list(T.K_RUNS), weights_sha256=r["sha"],
                                                              bn_layers=r["info"]))


# --------------------------------------------------------------------------- 4. the pipeline's rows

PIPELINE_FRAMES = (3, 10)      # the two frames of the launch with the fewest firing cells (10 and 12): every one of them is restated
_PIPE = {}


def _pipeline_expected(mode):
    """Per PIPELINE_FRAMES frame: rows [x, y, id] float64 from the decode of the restated logits + the restated RefineNet
    arg-max of every firing cell's patch."""
    if mode not in _PIPE:
        d, r = T.detector_regime(), T.refinenet_regime()
        loc, ids = T.restated_detector(mode, PIPELINE_FRAMES)
        kps = [O.pred_to_keypoints(torch.from_numpy(loc[j:j + 1]), torch.from_numpy(ids[j:j + 1]), 16)[0] for j in range(len(loc))]
        patches = np.concatenate([O.extract_patches(torch.from_numpy(d["images"][f][None]), kp).numpy()
                                  for f, kp in zip(PIPELINE_FRAMES, kps)])
        _, corners = N.refinenet_exact(r["sd"], patches, mode)
        rows, at = [], 0
        for j, kp in enumerate(kps):
            rows.append(_frame_rows(loc[j:j + 1], ids[j:j + 1], 16, corners[at:at + len(kp)]))
            at += len(kp)
        _PIPE[mode] = rows
    return _PIPE[mode]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS, indirect=True)
def test_pipeline_rows_on_trained_stats(dev, mode):
    """infer_batch, infer_image, infer_image_staged and one ResidentStream batch: rows == the decode of the restated logits + the
    restated RefineNet arg-max, on every firing cell of two frames."""
    from deepcharuco_amd.inference import infer_batch, infer_image, infer_image_staged
    from deepcharuco_amd.models.net import dcModel, lModel
    from deepcharuco_amd.models.refinenet import RefineNet, lRefineNet
    from deepcharuco_amd.stream import ResidentStream
    d, r = T.detector_regime(), T.refinenet_regime()
    exp = _pipeline_expected(mode)
    assert [e.shape[0] for e in exp] == [d["sharp"]["firing_per_frame"][f] for f in PIPELINE_FRAMES]
    dc, rn = lModel(dcModel(16, d["sd"], dev)), lRefineNet(RefineNet(r["sd"], dev))
    frames = d["frames"][list(PIPELINE_FRAMES)]
    res = infer_batch(frames, 16, dc, rn, kmax=96)
    rs = ResidentStream(16, dc, rn, batch=len(frames), height=64, width=96, kmax=96)
    streamed = [a for _, out in rs.run([torch.from_numpy(frames).to(dev)]) for a in out]
    for j, f in enumerate(PIPELINE_FRAMES):
        bgr = np.repeat(frames[j][..., None], 3, axis=2)
        assert _rows_equal(res[j], exp[j]), f"infer_batch frame {f}"
        assert _rows_equal(streamed[j], exp[j]), f"ResidentStream frame {f}"
        assert _rows_equal(infer_image(bgr, 16, dc, rn)[0], exp[j]), f"infer_image frame {f}"
        assert _rows_equal(infer_image_staged(bgr, 16, dc, rn)[0], exp[j]), f"infer_image_staged frame {f}"
    _report(f"trained_stats/pipeline/{_mode_id(mode)}", dict(frames=list(PIPELINE_FRAMES), corners=[int(e.shape[0]) for e in exp]))


# --------------------------------------------------------------------------- 5. confidences

def _check_conf_frames(res, plain, confs, frames_sel, loc, ids, dust_bin, what):
    """Rows and both confidences of the frames whose logits are restated; returns (worst ratio to the bound, corners,
    [min p, max p] of loc and ids)."""
    worst, corners, lo, hi = 0.0, 0, [1.0, 1.0], [0.0, 0.0]
    for j, f in enumerate(frames_sel):
        rows, zl, zi = T.expected_corners(loc[j:j + 1], ids[j:j + 1], dust_bin)
        assert rows.shape[0] > 0
        assert _rows_equal(res[f], rows), f"{what}: rows of frame {f}"
        assert plain is None or _rows_equal(plain[f], rows), f"{what}: rows of frame {f} without confidences"
        c = confs[f]
        assert c.shape == (rows.shape[0], 2) and c.dtype == np.float32
        for col, z in ((0, zl), (1, zi)):
            worst = max(worst, T.assert_conf_within_bound(np.ascontiguousarray(c[:, col]), z, f"{what}: frame {f} p_{'loc ids'.split()[col]}"))
            lo[col], hi[col] = min(lo[col], float(c[:, col].min())), max(hi[col], float(c[:, col].max()))
        corners += rows.shape[0]
    return worst, corners, [lo, hi]


@pytest.mark.parametrize("launch", ["B1", "B96"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS, indirect=True)
def test_confidences_are_the_softmax_of_the_restated_logits(dev, mode, launch):
    """Every corner's (p_loc, p_ids) of infer_batch(conf=True) against the float64 soft-max of the RESTATED logits of its cell
    -- the very bits the kernel holds -- within 2^-24 (3 sum |d_c| e^d_c / sum e^d_c + 32) relative: at B = 1 (3 work items, fewer
    than CUs: the small-prefetch tail) and in the 96-frame launch (288 items: the full-prefetch tail; frames 0 / 47 / 95 and the
    frame that holds the launch's sharpest corner, a probability within 1e-6 of 1).  Asking for confidences changes no row of
    any frame."""
    from deepcharuco_amd.inference import infer_batch
    from deepcharuco_amd.models.net import dcModel, lModel
    d = T.detector_regime()
    dc = lModel(dcModel(16, d["sd"], dev))
    loc, ids = T.restated_detector(mode)
    frames, sel = (d["frames"][:1], [0]) if launch == "B1" else (d["frames"], T.RESTATED)
    if launch == "B96":
        sharpest = d["sharp"]["sharpest_frame"]
        assert sharpest not in sel
        sel = sel + [sharpest]
        loc, ids = [np.concatenate([a, e]) for a, e in zip((loc, ids), T.restated_detector(mode, (sharpest,)))]
    plain = infer_batch(frames, 16, dc, None, kmax=96)
    res, confs = infer_batch(frames, 16, dc, None, kmax=96, conf=True)
    assert len(res) == len(plain) == len(frames) and all(_rows_equal(a, b) for a, b in zip(res, plain))
    assert [a.shape[0] for a in res] == d["sharp"]["firing_per_frame"][:len(frames)]
    worst, corners, span = _check_conf_frames(res, plain, confs, sel, loc[:len(sel)], ids[:len(sel)], 16, f"{launch} {_mode_id(mode)}")
    if launch == "B96":      # over the restated frames both heads have a winner under a half, and one comes within 1e-6 of 1
        assert max(span[0]) < 0.5 and max(span[1]) > 1 - 1e-6, span
    _report(f"trained_stats/confidence/{launch}_{_mode_id(mode)}", dict(corners=corners, worst_ratio_to_bound=worst, p_min=span[0], p_max=span[1]))


def test_confidences_at_the_head_width_edges(dev):
    """One set of restated features under ids heads of n_ids + 1 = 32, 33 and 64 rows (one full tile; a second tile whose only
    valid row is the dust bin; two full tiles), a caller's dust bin that is not n_ids (5 and 200), and a duplicated winning row
    (two equal largest terms: p_ids <= 0.5, the lower row wins): logits by bits, rows, and both confidences within the bound."""
    from deepcharuco_amd.inference import infer_batch
    from deepcharuco_amd.models.net import dcModel, lModel
    d = T.detector_regime()
    feats = T.restated_features(False)
    frames = d["frames"][T.RESTATED]
    rep = {}

    def run(tag, sd, n_ids, dust_bin):
        loc, ids = N.detector_heads(sd, feats)
        dc = lModel(dcModel(n_ids, sd, dev))
        out = dc.model.forward_u8(torch.from_numpy(frames).to(dev))
        T.assert_same_bits(out["loc"].cpu().numpy(), loc, f"{tag}: loc")
        T.assert_same_bits(out["ids"].cpu().numpy(), ids, f"{tag}: ids")
        plain = infer_batch(frames, dust_bin, dc, None, kmax=96)
        res, confs = infer_batch(frames, dust_bin, dc, None, kmax=96, conf=True)
        worst, corners, span = _check_conf_frames(res, plain, confs, [0, 1, 2], loc, ids, dust_bin, tag)
        rep[tag] = dict(corners=corners, worst_ratio_to_bound=worst, p_min=span[0], p_max=span[1])
        return res, confs, loc, ids

    for n_ids in (31, 32, 63):
        res, _, _, ids = run(f"n_ids{n_ids}", T.widen_ids_head(d["sd"], 16, n_ids), n_ids, n_ids)
        fired = np.concatenate([a[:, 2] for a in res])
        assert fired.max() >= 16, "none of the added rows wins a firing cell"
        if n_ids == 63:
            assert fired.max() >= 32, "no winner in the second ids tile"
        if n_ids == 32:
            assert (ids.argmax(1) == 32).any(), "the lone row of the second tile never wins"
    from deepcharuco_amd import _lib
    with pytest.raises(_lib.DcxError, match="DCX_E_NIDS"):      # 65 rows would need a third ids tile: refused at create()
        dcModel(64, T.widen_ids_head(d["sd"], 16, 64), dev)
    for db in (5, 200):
        res, _, _, ids = run(f"dust_bin{db}", d["sd"], 16, db)
        fired = np.concatenate([a[:, 2] for a in res])
        assert not (fired == db).any() and (fired == 16).any()        # class 16 is an ordinary id when it is not the dust bin
    a, b = 3, 4                 # the two rows sit in the two lane halves of one tile
    sd = {k: v.copy() for k, v in d["sd"].items()}
    sd["convDb.weight"][b], sd["convDb.bias"][b] = sd["convDb.weight"][a], sd["convDb.bias"][a]
    ids0 = N.detector_heads(sd, feats)[1]
    sd["convDb.bias"][[a, b]] += np.float32(np.quantile(np.delete(ids0, [a, b], axis=1).max(axis=1) - ids0[:, a], 0.7))
    res, confs, loc, ids = run("duplicated_row", sd, 16, 16)
    tied = (ids[:, a] == ids.max(axis=1)) & (ids[:, b] == ids[:, a])
    n_tied = 0
    for f in range(3):
        on = res[f][:, 2] == a
        assert not (res[f][:, 2] == b).any()
        cells = tied[f][res[f][on, 1] // 8, res[f][on, 0] // 8]
        assert cells.all()
        assert np.all(confs[f][on, 1] <= 0.5), confs[f][on, 1]
        n_tied += int(on.sum())
    assert n_tied >= 10, n_tied
    rep["duplicated_row"]["tied_firing_cells"] = n_tied
    _report("trained_stats/confidence/head_width_edges", rep)


# The 392x392 frame is compared with the live torch oracle (restating it would take tens of seconds; what it tests is the
# compaction's index, and a wrong index is a gross error).  Its probabilities follow the torch-fp32 logits, which differ from the
# kernel's: the bound is four times the largest |p(torch fp32) - p(float64)| over this frame's corners, measured on the CPU
# (1.208e-5; the logits differ by 6.5e-5 there, the sharpened heads' six times the usual gap).
CONF_392_ATOL = 4.84e-5


def test_compaction_with_confidences_beyond_one_super_chunk(dev):
    """One 392x392 frame: 2,401 cells, two super-chunks of the compaction (its count-first path and the gather of per-cell
    confidences by cell index), 983 corners, 153 of them in the second super-chunk.  Rows == the live oracle's exactly (no
    decision of this frame is closer than 1e-3 in float64, checked), confidences within CONF_392_ATOL.  With a pool smaller than
    the count the first `pool` slots hold the same rows and confidences, the count is still reported, and nothing is written
    past the pool (the buffer is prefilled); of two frames in a pool that holds only one of them, the complete one keeps its
    rows and confidences."""
    from deepcharuco_amd.corner_pool import views
    from deepcharuco_amd.inference import infer_batch, infer_batch_device, packed_len, unpack_results
    from deepcharuco_amd.models.net import dcModel, lModel
    d = T.detector_regime()
    frame = W.synthetic_frames("noise", 5106, 1, 392, 392)
    img = N.normalised(frame)
    l64, i64 = T.detector_logits64(d["sd"], img)
    for z in (l64, i64):
        s = np.sort(z, axis=1)
        assert (s[:, -1] - s[:, -2]).min() > 1e-3
    t_dc = O.to_torch_state_dict(d["sd"])
    loc, ids = O.detector_forward(t_dc, torch.from_numpy(img)[:, None])
    assert np.array_equal(T.firing(loc.numpy(), ids.numpy(), 16), T.firing(l64, i64, 16))
    kp, idf = O.pred_to_keypoints(loc, ids, 16)
    order = np.argsort(idf.numpy(), kind="stable")
    exp = O.infer_image(None, 16, t_dc, None, gray=frame[0])
    exp_c = O.keypoint_confidences(loc, ids, 16).numpy()
    total = exp.shape[0]
    fire = T.firing(l64, i64, 16).reshape(-1)
    assert fire.size == 2401 and total == int(fire.sum()) and fire[:2048].sum() > 100 and fire[2048:].sum() > 100
    dc = lModel(dcModel(16, d["sd"], dev))
    res, confs = infer_batch(frame, 16, dc, None, pool=1024, conf=True)
    assert _rows_equal(res[0], exp) and _rows_equal(infer_batch(frame, 16, dc, None, pool=1024)[0], exp)
    err = float(np.abs(confs[0] - exp_c[order]).max())
    print(f"392x392: {total} corners, confidences within {err:.3g} of the torch oracle (allowed {CONF_392_ATOL})")
    assert err <= CONF_392_ATOL, err
    # the pool's own layout, raster order: counts | starts | rows[pool][4] | xy[pool][2] | conf[pool][2]
    d_frame = torch.from_numpy(frame).to(dev)
    big = infer_batch_device(d_frame, 16, dc, None, pool=1024, conf=True).cpu().numpy()
    assert big[0] == total and big[1] == 0
    _, _, big_rows, _, big_conf = (v[:total] for v in views(big, 1, 1024))
    assert np.array_equal(big_rows[:, 3], np.flatnonzero(fire))                       # cell indices in raster order
    assert np.array_equal(big_rows[:, :2], kp.numpy()) and np.array_equal(big_rows[:, 2], idf.numpy())
    assert np.abs(big_conf - exp_c).max() <= CONF_392_ATOL
    sentinel, guard = -559038737, 256
    first = int(fire[:2048].sum())
    for pool in (first - 230, first + 70):      # the cut inside the first super-chunk, and inside the second
        assert 0 < pool < total
        n = packed_len(1, pool, True)
        buf = torch.full((n + guard,), sentinel, dtype=torch.int32, device=dev)
        infer_batch_device(d_frame, 16, dc, None, pool=pool, conf=True, out=buf[:n])
        torch.cuda.synchronize()
        a = buf.cpu().numpy()
        assert a[0] == total and a[1] == 0, (pool, a[:2])
        _, _, a_rows, _, a_conf = views(a[:n], 1, pool)
        assert np.array_equal(a_rows, big_rows[:pool]), pool
        assert np.array_equal(a_conf.view(np.int32), big_conf[:pool].view(np.int32)), pool
        assert np.all(a[2 + 4 * pool:2 + 6 * pool] == sentinel), f"pool={pool}: a row was written past the pool"
        assert np.all(a[n:] == sentinel), f"pool={pool}: a confidence was written past the pool"
    with pytest.warns(UserWarning, match=f"pool={total}"):
        again, confs2 = infer_batch(frame, 16, dc, None, pool=first - 230, conf=True)
    assert _rows_equal(again[0], exp) and np.array_equal(confs2[0], confs[0])
    # two frames in a pool that holds either of them but not both: the frame that was placed first is complete and keeps its
    # rows and confidences, the other is reported by its count only (which of the two finishes first is the hardware's choice)
    other = W.synthetic_frames("board", 5105, 1, 392, 392)
    l64b, i64b = T.detector_logits64(d["sd"], N.normalised(other))
    for z in (l64b, i64b):
        s = np.sort(z, axis=1)
        assert (s[:, -1] - s[:, -2]).min() > 4e-4
    exp_b = O.infer_image(None, 16, t_dc, None, gray=other[0])
    pair = np.concatenate([frame, other])
    full, full_c = infer_batch(pair, 16, dc, None, pool=2048, conf=True)
    assert _rows_equal(full[0], exp) and _rows_equal(full[1], exp_b) and np.array_equal(full_c[0], confs[0])
    pool = total + 17
    assert exp_b.shape[0] < pool < total + exp_b.shape[0]
    n = packed_len(2, pool, True)
    buf = torch.full((n + guard,), sentinel, dtype=torch.int32, device=dev)
    infer_batch_device(torch.from_numpy(pair).to(dev), 16, dc, None, pool=pool, conf=True, out=buf[:n])
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    part, counts, part_c = unpack_results(a[:n], 2, pool, False, True)
    assert counts.tolist() == [total, exp_b.shape[0]]
    complete = [r is not None for r in part]
    assert sum(complete) == 1, complete
    for f in range(2):
        if complete[f]:
            assert _rows_equal(part[f], full[f]) and np.array_equal(part_c[f], full_c[f]), f
    assert np.all(a[4 + 4 * pool:4 + 6 * pool] == sentinel) and np.all(a[n:] == sentinel)
    _report("trained_stats/confidence/392x392_two_super_chunks", dict(corners=total, in_second_super_chunk=int(fire[2048:].sum()),
                                                                      max_abs_err_vs_torch=err, allowed=CONF_392_ATOL,
                                                                      complete_frame_of_the_pair=int(np.argmax(complete))))
