"""ORACLE -- test infrastructure, NOT product code.

Both networks chained layer by layer through the exact-order restatements of oracle/conv_exact.c, so that the HIP path's
logits, heat-maps and arg-max decisions can be compared bit for bit (no tolerance, no near-tie exemption).

The layer tables follow deepcharuco_amd/csrc/dcx_api.hip (detector_run, refiner_run); which restatement a layer takes follows
family_of (dcx_conv_mfma.hip), restated in :func:`family_of`.  First layers (cin = 1) take the direct chain on the normalised
image, zero-padded after normalisation (dcx_first_dev.h: dcx_px_padded and dcx_conv1_quad, which dcx_misc.hip's dcx_conv1_kernel /
dcx_conv1_tile_kernel / dcx_conv1_patches_kernel all call).
The detector's convPa | convDa run on the GPU as one 512-channel layer; every output channel is independent, so restating the
two 256-channel halves separately gives the same bits.
"""
from __future__ import annotations

import numpy as np

from . import deepcharuco_oracle as O
from .conv_exact import conv_exact, heat_exact

DCX_CCH = 16      # dcx_conv_mfma.h: input channels per chunk
EPI = {"bnrelu": 0, "raw": 1, "heat": 2}

# (conv, bn, pad, pool) after conv1a, dcx_api.hip detector_run: steps[] then heads_a
DETECTOR_ENCODER = (("conv1b", "bn1b", 1), ("conv2a", "bn2a", 0), ("conv2b", "bn2b", 1), ("conv3a", "bn3a", 0),
                    ("conv3b", "bn3b", 1), ("conv4a", "bn4a", 0), ("conv4b", "bn4b", 0))
# (conv, bn, pad, ups-on-read, pool) after conv1a, dcx_api.hip refiner_run: steps[]; the head convPa reads conv5b up-sampled
REFINENET_BODY = (("conv1b", "bn1b", 0, 0, 0), ("conv2a", "bn2a", 0, 0, 0), ("conv2b", "bn2b", 0, 0, 1),
                  ("conv3a", "bn3a", 1, 0, 0), ("conv3b", "bn3b", 1, 0, 0), ("conv4a", "bn4a", 1, 1, 0),
                  ("conv4b", "bn4b", 1, 0, 0), ("conv5a", "bn5a", 1, 1, 0), ("conv5b", "bn5b", 1, 0, 0))


def family_of(cin, cout, ks, pool, epi, ups, deterministic):
    """dcx_conv_mfma.hip family_of: the summation order of a layer, from the layer and the process-wide mode only."""
    cout_pad = (cout + 3) // 4 * 4
    if deterministic or ks != 3 or epi == "raw" or cin < 2 * DCX_CCH:
        return "direct"
    if ups and not pool and (epi == "bnrelu" or (epi == "heat" and cout_pad == 64)):
        return "w2p"
    if epi == "bnrelu":
        return "w2h"
    return "direct"


def _bn(sd, bn):
    return [sd[f"{bn}.weight"], sd[f"{bn}.bias"], sd[f"{bn}.running_mean"], sd[f"{bn}.running_var"]]


def _np(sd):
    return {k: np.ascontiguousarray(np.asarray(v), np.float32) for k, v in sd.items()}


def first_layer(sd, images, pad):
    """conv1a + bn1a + ReLU of either network: images (N, H, W) normalised float32 -> (N, 64, H', W')."""
    x = np.ascontiguousarray(images, np.float32)[:, None]
    return conv_exact(x, sd["conv1a.weight"], sd["conv1a.bias"], _bn(sd, "bn1a"), pad=pad, family="direct")


def normalised(frames_u8, pix="gray"):
    """The first layer's load: gray, BGR (OpenCV 4.x constants) or BGR-legacy14 u8 frames -> pre_bgr_image (model_utils.py:46-50)."""
    f = np.asarray(frames_u8)
    if pix != "gray":
        f = O.bgr2gray(f, "opencv4" if pix == "bgr" else "legacy14")
    return np.stack([O.pre_bgr_image(g)[0] for g in f.reshape((-1,) + f.shape[-2:])])


def detector_layers(n, h, w, n_ids, deterministic):
    """[(name, family, pick args of dcx_conv_pick_name_ups)] of every MFMA launch of detector_run for an (n, h, w) batch."""
    out, cin, hh, ww = [], 64, h, w
    for conv, _, pool in DETECTOR_ENCODER:
        cout = 128 if conv in ("conv3a", "conv3b", "conv4a", "conv4b") else 64
        out.append((conv, family_of(cin, cout, 3, pool, "bnrelu", 0, deterministic), (n, cin, hh, ww, cout, 3, pool, 0, 0)))
        cin = cout
        if pool:
            hh, ww = hh // 2, ww // 2
    out.append(("convPa|convDa", family_of(128, 512, 3, 0, "bnrelu", 0, deterministic), (n, 128, hh, ww, 512, 3, 0, 0, 0)))
    cells = (h // 8) * (w // 8)
    out.append(("convPb", family_of(256, 65, 1, 0, "raw", 0, deterministic), (n, 256, 1, cells, 65, 1, 0, 1, 0)))
    out.append(("convDb", family_of(256, n_ids + 1, 1, 0, "raw", 0, deterministic), (n, 256, 1, cells, n_ids + 1, 1, 0, 1, 0)))
    return out


def detector_features(sd, images, deterministic):
    """Everything up to the two 1x1 heads: images (N, H, W) normalised float32 -> (convPa output, convDa output), NCHW."""
    sd = _np(sd)
    x = first_layer(sd, images, 1)
    for conv, bn, pool in DETECTOR_ENCODER:
        cin, cout = x.shape[1], sd[f"{conv}.weight"].shape[0]
        fam = family_of(cin, cout, 3, pool, "bnrelu", 0, deterministic)
        x = conv_exact(x, sd[f"{conv}.weight"], sd[f"{conv}.bias"], _bn(sd, bn), pad=1, pool=bool(pool), family=fam)
    fam = family_of(128, 512, 3, 0, "bnrelu", 0, deterministic)
    pa = conv_exact(x, sd["convPa.weight"], sd["convPa.bias"], _bn(sd, "bnPa"), pad=1, family=fam)
    da = conv_exact(x, sd["convDa.weight"], sd["convDa.bias"], _bn(sd, "bnDa"), pad=1, family=fam)
    return pa, da


def detector_heads(sd, feats):
    """convPb / convDb (net.py:74,77): raw 1x1 convolutions in the direct chain (dcx_tail.hip keeps the same order)."""
    sd = _np(sd)
    pa, da = feats
    loc = conv_exact(pa, sd["convPb.weight"], sd["convPb.bias"], None, pad=0, family="direct")
    ids = conv_exact(da, sd["convDb.weight"], sd["convDb.bias"], None, pad=0, family="direct")
    return loc, ids


def detector_exact(sd, frames, pix="gray", deterministic=False):
    """(loc (N,65,H/8,W/8), ids (N,n_ids+1,H/8,W/8)) float32, bit for bit what dcModel.forward / forward_u8 return.  frames:
    (N,H,W) u8 gray, (N,H,W,3) u8 BGR (pix = "bgr" / "legacy14"), or (N,H,W) float32 already normalised (pix = "f32")."""
    images = np.asarray(frames, np.float32) if pix == "f32" else normalised(frames, pix)
    return detector_heads(sd, detector_features(sd, images, deterministic))


def refinenet_layers(n, deterministic, head=None):
    """[(name, family, pick args)] of refiner_run's MFMA launches; the head's family unless DCX_FORCE_CFG picks it (head=)."""
    out, cin, hw = [], 64, 22
    for conv, _, pad, ups, pool in REFINENET_BODY:
        cout = 64 if conv in ("conv1b", "conv5a", "conv5b") else 128
        ho = (hw << ups) + 2 * pad - 2
        out.append((conv, family_of(cin, cout, 3, pool, "bnrelu", ups, deterministic), (n, cin, ho, ho, cout, 3, pool, 0, ups)))
        cin, hw = cout, ho // 2 if pool else ho
    out.append(("convPa+convPb", head or family_of(64, 64, 3, 0, "heat", 1, deterministic), None))
    return out


def refinenet_body(sd, patches, deterministic):
    """conv1a .. conv5b: patches (K,24,24) or (K,1,24,24) float32 -> (K, 64, 32, 32)."""
    sd = _np(sd)
    x = first_layer(sd, np.asarray(patches, np.float32).reshape(-1, 24, 24), 0)
    for conv, bn, pad, ups, pool in REFINENET_BODY:
        fam = family_of(x.shape[1], sd[f"{conv}.weight"].shape[0], 3, pool, "bnrelu", ups, deterministic)
        x = conv_exact(x, sd[f"{conv}.weight"], sd[f"{conv}.bias"], _bn(sd, bn), pad=pad, ups=bool(ups), pool=bool(pool), family=fam)
    return x


def refinenet_head(sd, body, order):
    sd = _np(sd)
    return heat_exact(body, sd["convPa.weight"], sd["convPa.bias"], _bn(sd, "bnPa"), sd["convPb.weight"],
                      sd["convPb.bias"].reshape(-1)[0], order)


def first_flat_argmax(heat):
    """speedy_bargmax2d (model_utils.py:39-43): (K,1,64,64) -> (K,2) int64 (col, row) of the first flat maximum."""
    flat = heat.reshape(heat.shape[0], -1)
    idx = np.argmax(flat, axis=1)
    return np.stack([idx % heat.shape[-1], idx // heat.shape[-1]], axis=1).astype(np.int64)


def refinenet_exact(sd, patches, deterministic=False, head=None):
    """(heat (K,1,64,64) float32, corners (K,2) int64) bit for bit what RefineNet.forward / infer_patches compute.  head: the
    head's order when DCX_FORCE_CFG pins a HEAT instantiation ("direct" / "w2p"); default: family_of."""
    order = head or family_of(64, 64, 3, 0, "heat", 1, deterministic)
    heat = refinenet_head(sd, refinenet_body(sd, patches, deterministic), order)
    return heat, first_flat_argmax(heat)
