"""Both networks, bit for bit, against the layer-chained exact restatement (oracle/net_exact.py).

Every MFMA layer is pinned on its own by test_gpu_parity.py; here the whole chain is: the first layers (dcx_conv1_kernel<PX,1>,
dcx_conv1_tile_kernel, dcx_conv1_patches_kernel and, in the switch sweep, dcx_conv1_kernel<PX,4>), the RefineNet head of both
families with its per-tile arg-max and dcx_refine_finalize_kernel, and the fused tail's arg-max merges.  Every comparison is
exact: logits and heat-maps by their bits, arg-max decisions on every cell and patch, with no near-tie exemption.
test_exact_chain_host.py ties the restatement to float64 maths and to the reference's fixtures."""
import hashlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import REPO, GoldenCase
from deepcharuco_amd import weights as W
from oracle import deepcharuco_oracle as O
from oracle import net_exact as N

pytestmark = pytest.mark.gpu

MODES = [False, True]
MODE_IDS = ["default", "deterministic"]
HEAT_CFGS = {"direct": "dcx_conv_mfma_kernel<DcxConvCfg<1,4,2,2,8,32,3,0,DCX_EPI_HEAT>>",
             "w2p": "dcx_conv_wino2p_kernel<DcxWino2pCfg<8,16,DCX_EPI_HEAT,1>>"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def tiny():
    return GoldenCase("tiny_noise_64x96")


@pytest.fixture
def mode(request):
    """set_deterministic(param) for the test, default mode afterwards; DCX_FORCE_CFG is never inherited."""
    from deepcharuco_amd.inference import set_deterministic
    os.environ.pop("DCX_FORCE_CFG", None)
    set_deterministic(request.param)
    yield request.param
    set_deterministic(False)


def _family(kernel_name):
    return "w2p" if "wino2p" in kernel_name else "w2h" if "wino2h" in kernel_name else "direct"


def _same_bits(got, exp):
    got, exp = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(exp, np.float32)
    assert got.shape == exp.shape
    return int((got.view(np.uint32) != exp.view(np.uint32)).sum())


def _frame_rows(loc1, ids1, n_ids, kpts_corners=None):
    """infer_image's rows for one frame from ITS logits (1,C,hc,wc): [x, y, id] sorted by id (stable), int64; with the refined
    corners (K,2) (raster order) float64 (corners - 32) / 8 + key-point, as refinenet.py:108-114 computes it."""
    kp, idf = O.pred_to_keypoints(torch.from_numpy(loc1), torch.from_numpy(ids1), n_ids)
    if idf.shape[0] == 0:
        return np.array([])
    xy = kp.numpy()
    if kpts_corners is not None:
        xy = ((torch.from_numpy(kpts_corners) - 32) / 8 + kp).numpy()
    order = np.argsort(idf.numpy(), kind="stable")
    out = np.empty((idf.shape[0], 3), np.float64 if kpts_corners is not None else np.int64)
    out[:, :2] = xy
    out[:, 2] = idf.numpy()
    return out[order]


def _rows_equal(got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    return got.shape == exp.shape and got.dtype == exp.dtype and np.array_equal(got, exp)


# --------------------------------------------------------------------------- 1. detector logits

DET_SIZES = [(64, 96), (67, 101), (9, 15), (8, 8), (100, 75), (136, 200)]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS, indirect=True)
def test_detector_logits_bit_exact(dev, tiny, mode):
    """forward_u8 and forward (f32) == detector_exact, every logit, at B = 1 over sizes with partial first-layer tiles and the
    split-position Winograd shapes, a B = 48 launch (dcx_conv1_kernel<PX,1>; three frames restated) and a 240x320 fixture frame.
    The family of every launch is the restated one (dcx_conv_pick_name_ups)."""
    from deepcharuco_amd import _lib
    from deepcharuco_amd.models.net import dcModel
    L = _lib.lib()
    dc = dcModel(tiny.n_ids, tiny.sd_dc, dev)
    big = GoldenCase("noise_240x320")
    dc_big = dcModel(big.n_ids, big.sd_dc, dev)
    runs = [(dc, tiny.sd_dc, W.synthetic_frames("noise", 700 + i, 1, h, w), None) for i, (h, w) in enumerate(DET_SIZES)]
    runs.append((dc, tiny.sd_dc, W.synthetic_frames("board", 801, 48, 64, 96), [0, 23, 47]))
    runs.append((dc_big, big.sd_dc, big.frame[None], None))
    for model, sd, frames, sel in runs:
        n, h, w = frames.shape
        for name, fam, args in N.detector_layers(n, h, w, model.n_ids, mode):
            picked = L.dcx_conv_pick_name_ups(*args).decode()
            assert _family(picked) == fam, (name, (h, w, n), picked, fam)
        out = model.forward_u8(torch.from_numpy(frames).to(dev))
        out_f = model.forward(torch.from_numpy(N.normalised(frames)[:, None]).to(dev))
        sel = list(range(n)) if sel is None else sel
        loc, ids = N.detector_exact(sd, frames[sel], deterministic=mode)
        for key, exp in (("loc", loc), ("ids", ids)):
            for tag, o in (("u8", out), ("f32", out_f)):
                nbad = _same_bits(o[key].cpu().numpy()[sel], exp)
                assert nbad == 0, f"{key} ({tag}) {n}x{h}x{w}: {nbad} of {exp.size} logits differ from the restatement"


# --------------------------------------------------------------------------- 2. RefineNet heat

K_RUNS = {1: [0], 16: list(range(16)), 113: [0, 57, 100, 112], 600: [0, 311, 512, 599]}


def _patch_pool(case, k):
    """k patches of a fixture frame around key-points all over it, the borders included (zero padding inside the patch)."""
    rng = np.random.default_rng(77)
    h, w = case.frame.shape
    kp = np.stack([rng.integers(0, w, k), rng.integers(0, h, k)], 1)
    kp[:4] = [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]]
    x = torch.from_numpy(O.pre_bgr_image(case.frame))
    return O.extract_patches(x, torch.from_numpy(kp)).numpy(), kp


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS, indirect=True)
def test_refinenet_heat_bit_exact(dev, mode, monkeypatch):
    """RefineNet.forward == refinenet_exact at K = 1, 16, 113, 600 (the f32 first layer's launch rule changes at K >= 512),
    under the family rule and with DCX_FORCE_CFG pinning each HEAT instantiation; infer_patches' corners and xy == the
    restated first flat arg-max on every restated patch."""
    from deepcharuco_amd.models.refinenet import RefineNet
    case = GoldenCase("board_240x320")
    rn = RefineNet(case.sd_rn, dev)
    pool, kp = _patch_pool(case, 600)
    sel = sorted({i for v in K_RUNS.values() for i in v})
    body = N.refinenet_body(case.sd_rn, pool[sel], mode)
    natural = N.family_of(64, 64, 3, 0, "heat", 1, mode)
    exp = {o: N.refinenet_head(case.sd_rn, body, o) for o in ("direct", "w2p")}
    pos = {i: j for j, i in enumerate(sel)}
    for head in (None, "direct", "w2p"):
        if head is None:
            monkeypatch.delenv("DCX_FORCE_CFG", raising=False)
        else:
            monkeypatch.setenv("DCX_FORCE_CFG", HEAT_CFGS[head])
        order = head or natural
        for k, idx in K_RUNS.items():
            p = torch.from_numpy(pool[:k]).to(dev)
            heat = rn(p[:, None]).cpu().numpy()
            e = exp[order][[pos[i] for i in idx]]
            nbad = _same_bits(heat[idx], e)
            assert nbad == 0, f"K={k}, head {order}: {nbad} heat values differ"
            cog, c = rn.infer_patches(p, torch.from_numpy(kp[:k]).to(dev))
            ec = N.first_flat_argmax(e)
            assert np.array_equal(c.cpu().numpy()[idx], ec), f"K={k}, head {order}: corners"
            exy = ((torch.from_numpy(ec) - 32) / 8 + torch.from_numpy(kp[idx])).numpy()
            assert np.array_equal(cog.cpu().numpy()[idx], exy)
    monkeypatch.delenv("DCX_FORCE_CFG", raising=False)


# --------------------------------------------------------------------------- 3. heat ties

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS, indirect=True)
def test_heat_argmax_ties(dev, mode, monkeypatch):
    """Exactly tied heat maxima across tiles, phases and waves: constant patches (both ends of the normalised range) and a head
    whose convPb.weight is zero (heat == bias everywhere: corner (0, 0), xy = key-point - 4).  The first flat maximum wins."""
    from deepcharuco_amd.models.refinenet import RefineNet
    sd = W.synthetic_state_dict("refinenet", 2)
    vals = np.float32([(0 - 128) / 255, (255 - 128) / 255, 0.0, (77 - 128) / 255])
    const = np.ascontiguousarray(np.broadcast_to(vals[:, None, None], (4, 24, 24)))
    sd0 = dict(sd)
    sd0["convPb.weight"] = np.zeros_like(sd["convPb.weight"])
    kp = np.array([[5, 7], [100, 3], [0, 0], [319, 239]])
    body = N.refinenet_body(sd, const, mode)
    body0 = N.refinenet_body(sd0, const, mode)
    for head in ("direct", "w2p"):
        monkeypatch.setenv("DCX_FORCE_CFG", HEAT_CFGS[head])
        e = N.refinenet_head(sd, body, head)
        n_max = [int((r == r.max()).sum()) for r in e.reshape(4, -1)]
        assert max(n_max) > 1, n_max          # the (255 - 128) / 255 patch has several equal maxima in both orders
        e0 = N.refinenet_head(sd0, body0, head)
        assert np.all(e0 == np.float32(sd["convPb.bias"][0]))
        for model_sd, exp in ((sd, e), (sd0, e0)):
            rn = RefineNet(model_sd, dev)
            p = torch.from_numpy(const).to(dev)
            assert _same_bits(rn(p[:, None]).cpu().numpy(), exp) == 0, head
            cog, c = rn.infer_patches(p, torch.from_numpy(kp).to(dev))
            ec = N.first_flat_argmax(exp)
            assert np.array_equal(c.cpu().numpy(), ec), (head, c.cpu().numpy(), ec, n_max)
            assert np.array_equal(cog.cpu().numpy(), ((torch.from_numpy(ec) - 32) / 8 + torch.from_numpy(kp)).numpy())
        assert np.array_equal(c.cpu().numpy(), np.zeros((4, 2), np.int64))
        assert np.array_equal(cog.cpu().numpy(), (kp - 4).astype(np.float32))
    monkeypatch.delenv("DCX_FORCE_CFG", raising=False)


# --------------------------------------------------------------------------- 4. fused-tail ties

# (head, cout a, cout b, n_ids): b's 1x1 row (weight and bias) is a copy of a's, so the two logits are equal bit for bit
TAIL_TIES = [("loc", 3, 4, 16),     # across the lane halves of one wave
             ("loc", 31, 32, 16),   # across waves 0 / 1
             ("loc", 63, 64, 16),   # against the no-corner class (wave 1 / wave 2)
             ("ids", 15, 16, 16),   # against the dust bin
             ("ids", 31, 32, 40)]   # across the two ids tiles


@pytest.mark.parametrize("tie", TAIL_TIES, ids=[f"{t[0]}{t[1]}_{t[2]}_n{t[3]}" for t in TAIL_TIES])
def test_fused_tail_ties(dev, tiny, tie):
    """Detector weights with a duplicated 1x1 row, its bias raised until the pair wins most cells: ids and integer cells of
    infer_batch, infer_image (fused tail) and infer_image_staged (stand-alone decode) == the decode of the restated logits, on
    every cell; the lower cout of a tied pair wins."""
    from deepcharuco_amd.inference import infer_batch, infer_image, infer_image_staged
    from deepcharuco_amd.models.net import dcModel, lModel
    head, a, b, n_ids = tie
    frames = np.concatenate([tiny.frame[None], W.synthetic_frames("board", 903, 1, 64, 96)])
    sd = {k: v.copy() for k, v in tiny.sd_dc.items()}
    if n_ids != tiny.n_ids:        # more ids rows over the same backbone
        rng = np.random.default_rng(n_ids)
        w0, b0 = sd["convDb.weight"], sd["convDb.bias"]
        extra = (rng.standard_normal((n_ids + 1 - w0.shape[0],) + w0.shape[1:]) * w0.std()).astype(np.float32)
        sd["convDb.weight"] = np.concatenate([w0[:-1], extra, w0[-1:]])
        sd["convDb.bias"] = np.concatenate([b0[:-1], (rng.standard_normal(extra.shape[0]) * b0[:-1].std()).astype(np.float32), b0[-1:]])
    feats = N.detector_features(sd, N.normalised(frames), False)
    conv = "convPb" if head == "loc" else "convDb"
    sd[f"{conv}.weight"][b] = sd[f"{conv}.weight"][a]
    sd[f"{conv}.bias"][b] = sd[f"{conv}.bias"][a]
    logits = N.detector_heads(sd, feats)[0 if head == "loc" else 1]
    others = np.delete(logits, [a, b], axis=1).max(axis=1)
    sd[f"{conv}.bias"][[a, b]] += np.float32(np.quantile(others - logits[:, a], 0.7))
    if head == "loc":
        sd["convDb.bias"][n_ids] -= 50.0       # every cell's id fires unless loc says "no corner"
    else:
        sd["convPb.bias"][64] -= 50.0          # loc never says "no corner"
        if b != n_ids:
            sd["convDb.bias"][n_ids] -= 50.0
    loc, ids = N.detector_heads(sd, feats)
    lg = loc if head == "loc" else ids
    tied = int(((lg[:, a] == lg.max(axis=1)) & (lg[:, b] == lg[:, a])).sum())
    print(f"{tie}: {tied} tied cells of {lg[:, 0].size}")
    assert tied > 0.3 * lg[:, 0].size
    dc = lModel(dcModel(n_ids, sd, dev))
    out = dc.model.forward_u8(torch.from_numpy(frames).to(dev))
    assert _same_bits(out["loc"].cpu().numpy(), loc) == 0 and _same_bits(out["ids"].cpu().numpy(), ids) == 0
    res = infer_batch(frames, n_ids, dc)
    for f in range(len(frames)):
        exp = _frame_rows(loc[f:f + 1], ids[f:f + 1], n_ids)
        assert exp.shape[0] > 0
        bgr = np.repeat(frames[f][..., None], 3, axis=2)
        assert _rows_equal(res[f], exp), f"infer_batch frame {f}"
        assert _rows_equal(infer_image(bgr, n_ids, dc)[0], exp), f"infer_image frame {f}"
        assert _rows_equal(infer_image_staged(bgr, n_ids, dc)[0], exp), f"infer_image_staged frame {f}"


# --------------------------------------------------------------------------- 5. the pipeline's fused patch gather

@pytest.mark.parametrize("pix", ["gray", "bgr", "legacy14"])
def test_pipeline_patch_gather_bit_exact(dev, tiny, pix):
    """infer_batch on weights where every cell fires (corners in the border cells): ids == the restated decode on every cell, xy
    == the restated RefineNet arg-max on oracle-gathered patches for selected corners, the four frame corners included
    (dcx_conv1_patches_kernel reads the frames directly, in gray / BGR / BGR-legacy14)."""
    from deepcharuco_amd.inference import infer_batch
    from deepcharuco_amd.models.net import dcModel, lModel
    from deepcharuco_amd.models.refinenet import RefineNet, lRefineNet
    sd = {k: v.copy() for k, v in tiny.sd_dc.items()}
    sd["convDb.bias"][tiny.n_ids] -= 50.0
    sd["convPb.bias"][64] -= 50.0
    rng = np.random.default_rng(31)
    frames = rng.integers(0, 256, (2, 64, 96, 3), dtype=np.uint8) if pix != "gray" else W.synthetic_frames("board", 905, 2, 64, 96)
    if pix != "gray":
        assert not np.array_equal(O.bgr2gray(frames, "opencv4"), O.bgr2gray(frames, "legacy14"))
    dc = lModel(dcModel(tiny.n_ids, sd, dev))
    rn = lRefineNet(RefineNet(tiny.sd_rn, dev))
    res = infer_batch(frames, tiny.n_ids, dc, rn, kmax=128, **({} if pix == "gray" else {"bgr_variant": "opencv4" if pix == "bgr" else pix}))
    images = N.normalised(frames, pix)
    loc, ids = N.detector_exact(sd, frames, pix=pix)
    for f in range(len(frames)):
        kp, idf = O.pred_to_keypoints(torch.from_numpy(loc[f:f + 1]), torch.from_numpy(ids[f:f + 1]), tiny.n_ids)
        hc, wc = loc.shape[2:]
        assert kp.shape[0] == hc * wc                       # every cell fires
        cells = [0, wc - 1, (hc - 1) * wc, hc * wc - 1, 13, 50]
        patches = O.extract_patches(torch.from_numpy(images[f][None]), kp[cells]).numpy()
        _, corners = N.refinenet_exact(tiny.sd_rn, patches, False)
        order = np.argsort(idf.numpy(), kind="stable")
        got = res[f]
        assert got.shape == (hc * wc, 3) and np.array_equal(got[:, 2], idf.numpy()[order])
        where = {int(c): j for j, c in enumerate(order)}
        for c, cr in zip(cells, corners):
            exy = ((torch.from_numpy(cr) - 32) / 8 + kp[c]).numpy().astype(np.float64)
            assert np.array_equal(got[where[c], :2], exy), (pix, f, c, got[where[c]], exy)


# --------------------------------------------------------------------------- 6. the detector's first layer in every pixel format

PIX_IDS = {"gray": 0, "bgr": 1, "legacy14": 2}            # DCX_PIX_GRAY8 / DCX_PIX_BGR8 / DCX_PIX_BGR8_LEGACY14
# (B, H, W, restated frames): one partial 16x16 tile; 2x3 tiles with the image index folded into blockIdx.y (both
# dcx_conv1_tile_kernel, or dcx_conv1_kernel<PX,4> under DCX_CONV1_TILE=0); gx * gy = 1024 is not < 1024: dcx_conv1_kernel<PX,1>
FRONT_SHAPES = [(1, 9, 15, [0]), (2, 17, 33, [0, 1]), (1024, 8, 9, [0, 511, 1023])]


def _windowed_frames(pix, b, h, w, seed):
    """(frames (B,H,W[,3]) u8, buffer, byte offset, frame stride, pitch): the frames as windows of a larger byte buffer whose
    other bytes are 255 (pitch = W bpp + 5, frame stride = pitch (H + 1) + 3, offset 7).  Colour pixels are drawn from the
    committed colours on which the two OpenCV generations give different gray levels."""
    rng = np.random.default_rng(seed)
    if pix == "gray":
        frames = rng.integers(0, 256, (b, h, w), dtype=np.uint8)
    else:
        differ = np.load(os.path.join(REPO, "tests", "golden", "bgr2gray_formula.npz"))["bgr_differ"].reshape(-1, 3)
        frames = differ[rng.integers(0, differ.shape[0], (b, h, w))]
    bpp = 1 if pix == "gray" else 3
    pitch, off = w * bpp + 5, 7
    stride = pitch * (h + 1) + 3
    buf = np.full(off + b * stride, 255, np.uint8)
    for f in range(b):
        rows = buf[off + f * stride: off + f * stride + h * pitch].reshape(h, pitch)
        rows[:, :w * bpp] = frames[f].reshape(h, w * bpp)
    return np.ascontiguousarray(frames), buf, off, stride, pitch


def _front_act(det, buf, off, stride, pitch, pix, b, h, w, dev):
    """dcx_detector_front on the windowed frames -> conv1a's output (B, 64, H, W) float32, read from the front set's act offset
    (0), where it lies as C4 [B][16][H W][4]."""
    from deepcharuco_amd import _lib
    L = _lib.lib()
    nb = L.dcx_front_bytes(det.handle, b, h, w)
    assert nb >= b * 64 * h * w * 4
    front = torch.full((nb,), 0xA5, dtype=torch.uint8, device=dev)
    d = torch.from_numpy(buf).to(dev)
    rc = L.dcx_detector_front(det.handle, d.data_ptr() + off, stride, pitch, PIX_IDS[pix], b, h, w, front.data_ptr(), nb,
                              _lib.current_stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    c4 = front[:b * 64 * h * w * 4].view(torch.float32).reshape(b, 16, h * w, 4)
    return c4.permute(0, 1, 3, 2).reshape(b, 64, h, w).cpu().numpy()


_FRONT_SCRIPT = r"""
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np, torch
import test_gpu_exact_chain as T
from conftest import GoldenCase
from deepcharuco_amd.models.net import dcModel
c = GoldenCase("tiny_noise_64x96")
dev = torch.device("cuda", 0)
dc = dcModel(c.n_ids, c.sd_dc, dev)
out = {{}}
for i, (b, h, w, _) in enumerate(T.FRONT_SHAPES[:2]):
    for pix in T.PIX_IDS:
        _, buf, off, stride, pitch = T._windowed_frames(pix, b, h, w, 640 + i)
        out["%s_%d" % (pix, i)] = T._front_act(dc, buf, off, stride, pitch, pix, b, h, w, dev)
np.savez({outputs!r}, **out)
print("FRONT ok")
"""


def test_detector_first_layer_bit_exact_in_every_pixel_format(dev, tiny, tmp_path):
    """conv1a + bn1a + ReLU as dcx_detector_front leaves it == first_layer(normalised(frames, pix), pad 1), every value by its
    bits, in gray / BGR / BGR-legacy14, at the shapes that reach dcx_conv1_tile_kernel and dcx_conv1_kernel<PX,1>; the first two
    shapes once more in a child process under DCX_CONV1_TILE=0 (dcx_conv1_kernel<PX,4>).  The frames are windows of a larger
    buffer full of 255, so a wrong bytes-per-pixel, pitch or stride shows; their colours are ones on which the two OpenCV
    generations differ, and the two expected outputs do differ, so a swapped format cannot pass."""
    from deepcharuco_amd.models.net import dcModel
    dc = dcModel(tiny.n_ids, tiny.sd_dc, dev)
    sd = N._np(tiny.sd_dc)
    expect = {}
    for i, (b, h, w, sel) in enumerate(FRONT_SHAPES):
        for pix in PIX_IDS:
            frames, buf, off, stride, pitch = _windowed_frames(pix, b, h, w, 640 + i)
            exp = expect[pix, i] = N.first_layer(sd, N.normalised(frames[sel], pix), pad=1)
            got = _front_act(dc, buf, off, stride, pitch, pix, b, h, w, dev)
            assert got.shape == (b, 64, h, w)
            nbad = _same_bits(got[sel], exp)
            assert nbad == 0, f"{pix} {b}x{h}x{w}: {nbad} of {exp.size} values differ from the restatement"
        assert _same_bits(expect["bgr", i], expect["legacy14", i]) > 0, (b, h, w)
    outputs = str(tmp_path / "front_outputs.npz")
    script = _FRONT_SCRIPT.format(repo=REPO, tests=os.path.join(REPO, "tests"), outputs=outputs)
    env = dict(os.environ)
    env["DCX_CONV1_TILE"] = "0"
    out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "FRONT ok" in out.stdout, f"DCX_CONV1_TILE=0 (rc {out.returncode}): {out.stderr[-2000:]}"
    child = np.load(outputs)
    for i, (b, h, w, _) in enumerate(FRONT_SHAPES[:2]):
        for pix in PIX_IDS:
            nbad = _same_bits(child[f"{pix}_{i}"], expect[pix, i])
            assert nbad == 0, f"DCX_CONV1_TILE=0, {pix} {b}x{h}x{w}: {nbad} of {expect[pix, i].size} values differ from the restatement"


# --------------------------------------------------------------------------- 7. runtime switch sweep

_SWEEP_SCRIPT = r"""
import hashlib, sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np, torch
from conftest import GoldenCase
from deepcharuco_amd.inference import infer_batch
from deepcharuco_amd.models.net import dcModel, lModel
from deepcharuco_amd.models.refinenet import RefineNet, lRefineNet
c = GoldenCase("tiny_noise_64x96")
dev = torch.device("cuda", 0)
frames = np.load({inputs!r})
dc = lModel(dcModel(c.n_ids, c.sd_dc, dev)); rn = lRefineNet(RefineNet(c.sd_rn, dev))
out = dc.model.forward_u8(torch.from_numpy(frames["frames"]).to(dev))
heat = rn.model(torch.from_numpy(frames["patches"]).to(dev)[:, None])
rows = infer_batch(frames["frames"], c.n_ids, dc, rn)
torch.cuda.synchronize()
h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
print("SWEEP", h(out["loc"].cpu().numpy()), h(out["ids"].cpu().numpy()), h(heat.cpu().numpy()), h(np.concatenate([np.asarray(r, np.float64).reshape(-1, 3) for r in rows])))
"""

SWEEP = [("DCX_CONV1_TILE", "0"), ("DCX_W2HS", "0"), ("DCX_W2PS", "0"), ("DCX_CT_OUTER", "0"), ("DCX_CT_OUTER", "1"),
         ("DCX_XCD_WALK", "0"), ("DCX_OCC", "1"), ("DCX_DETERMINISTIC", "1")]


def test_runtime_switch_sweep(dev, tiny, tmp_path):
    """Each runtime switch in its own process (they are read once per process): the detector's logits, RefineNet's heat and the
    pipeline's corner rows hash to the restatement's for that mode (one 64x96 frame, 16 patches: single-round launches, where
    the split-position Winograd shapes and the first layer's tile kernel run)."""
    frames = tiny.frame[None]
    patches, _ = _patch_pool(tiny, 16)
    inputs = str(tmp_path / "sweep_inputs.npz")
    np.savez(inputs, frames=frames, patches=patches)
    h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    expect = {}
    for det in (False, True):
        loc, ids = N.detector_exact(tiny.sd_dc, frames, deterministic=det)
        heat, _ = N.refinenet_exact(tiny.sd_rn, patches, det)
        kp, _ = O.pred_to_keypoints(torch.from_numpy(loc), torch.from_numpy(ids), tiny.n_ids)
        p = O.extract_patches(torch.from_numpy(N.normalised(frames)), kp).numpy()
        _, corners = N.refinenet_exact(tiny.sd_rn, p, det)
        rows = _frame_rows(loc, ids, tiny.n_ids, corners)
        expect[det] = [h(loc), h(ids), h(heat), h(np.asarray(rows, np.float64).reshape(-1, 3))]
    script = _SWEEP_SCRIPT.format(repo=REPO, tests=os.path.join(REPO, "tests"), inputs=inputs)
    for var, val in SWEEP:
        env = dict(os.environ)
        env.pop("DCX_FORCE_CFG", None)
        env[var] = val
        t0 = time.time()
        out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=240)
        line = [l for l in out.stdout.splitlines() if l.startswith("SWEEP")]
        assert out.returncode == 0 and line, f"{var}={val} (rc {out.returncode}): {out.stderr[-2000:]}"
        got = line[0].split()[1:]
        exp = expect[var == "DCX_DETERMINISTIC"]
        for what, g, e in zip(("loc", "ids", "heat", "rows"), got, exp):
            assert g == e, f"{var}={val}: {what} differs from the restatement ({time.time() - t0:.1f} s)"
