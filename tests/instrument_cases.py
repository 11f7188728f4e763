"""What the profile hooks of the library must record, derived from the ORACLE's two networks and from include/deepcharuco_amd.h --
never from the library (tests/test_instrument_host.py, tests/test_gpu_instrument.py).  Importable without a GPU.

* ``trace_layers`` runs ``oracle.deepcharuco_oracle``'s ``detector_forward`` / ``refinenet_forward`` on shape-only tensors with a
  recording stand-in for ``torch.nn.functional`` and returns one ``Layer`` per ``conv2d``: channels, kernel size and padding as the
  oracle passed them, the convolution's own input and output size, whether its input came out of an ``interpolate`` (up-sampling
  on the read) and whether its output goes into a ``max_pool2d`` (pooling in the epilogue).
* ``flops`` of a layer is 2 * cout * cin * ks^2 * Ho * Wo with Ho x Wo the convolution's own output: after the up-sampling, before
  the pooling.
* ``expected_*`` turn the layers into the records the header documents for a call (launch order; which layers share a launch;
  which launches are hipEvent brackets with flops 0; n_images; the limited flag).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
import torch.nn.functional as F

from deepcharuco_amd import weights as W
from oracle import deepcharuco_oracle as O

# ids of the launches outside the convolution table (include/deepcharuco_amd.h, dcx_profile_kernel_name)
PROF_CONV1A, PROF_PATCHES, PROF_TAIL, PROF_FINALIZE = 100, 101, 102, 103
BRACKET_IDS = (PROF_CONV1A, PROF_PATCHES, PROF_TAIL, PROF_FINALIZE)
CLK_SLOTS, CLK_WORDS = 1024, 64          # the header: the first 1,024 records of a session own 64 probe words each
EPI_BNRELU, EPI_RAW, EPI_HEAT = 0, 1, 2  # dcx_conv_pick_name's epi argument
E_ARG = -1
DESIGN_GFLOP_PER_FRAME = 26.816          # a 320x240 frame with 16 corners
HEAT_PICK_N = 1 << 20                    # the fused head's tiling is chosen for "many patches", whatever the launch holds


@dataclass(frozen=True)
class Layer:
    name: str
    cin: int
    cout: int
    ks: int
    pad: int
    hin: int       # the convolution's own input (after an up-sampling)
    win: int
    ho: int        # the convolution's own output (before a pooling)
    wo: int
    ups: int
    pool: int
    bn: bool

    @property
    def flops(self) -> int:
        return 2 * self.cout * self.cin * self.ks * self.ks * self.ho * self.wo


class _RecordingF:
    """Stands in for ``torch.nn.functional`` inside the oracle module while a network runs."""

    def __init__(self, names):
        self.names, self.events, self.keep = names, [], []

    def _out(self, kind, x, y, **kw):
        self.keep += [x, y]                       # ids stay unique while the trace lives
        self.events.append(dict(kind=kind, src=id(x), dst=id(y), **kw))
        return y

    def conv2d(self, x, w, b=None, stride=1, padding=0):
        assert stride == 1
        y = F.conv2d(x, w, b, stride=stride, padding=padding)
        return self._out("conv", x, y, name=self.names[id(w)], cin=w.shape[1], cout=w.shape[0], ks=w.shape[2], pad=int(padding),
                         hin=x.shape[2], win=x.shape[3], ho=y.shape[2], wo=y.shape[3])

    def batch_norm(self, x, *a, **kw):
        return self._out("bn", x, F.batch_norm(x, *a, **kw))

    def relu(self, x):
        return self._out("same", x, F.relu(x))

    def max_pool2d(self, x, k, s):
        assert (k, s) == (2, 2)
        return self._out("pool", x, F.max_pool2d(x, k, s))

    def interpolate(self, x, scale_factor=None, mode=None):
        assert (scale_factor, mode) == (2, "nearest")
        return self._out("up", x, F.interpolate(x, scale_factor=scale_factor, mode=mode))


def trace_layers(net: str, h: int, w: int, n_ids: int = 16) -> List[Layer]:
    """The conv layers of the oracle's ``net`` ("detector" on an h x w frame, "refinenet" on its 24x24 patch), in call order."""
    sd_np = W.synthetic_state_dict(net, 1, n_ids) if net == "detector" else W.synthetic_state_dict(net, 1)
    sd = {k: torch.empty(v.shape, dtype=torch.float32, device="meta") for k, v in sd_np.items()}
    rec = _RecordingF({id(v): k[:-len(".weight")] for k, v in sd.items() if k.endswith(".weight")})
    x = torch.empty((1, 1, h, w) if net == "detector" else (1, 1, 24, 24), dtype=torch.float32, device="meta")
    real = O.F
    O.F = rec
    try:
        (O.detector_forward if net == "detector" else O.refinenet_forward)(sd, x)
    finally:
        O.F = real
    ev = rec.events
    produced = {e["dst"]: e for e in ev}
    consumers = {}
    for e in ev:
        consumers.setdefault(e["src"], []).append(e)

    def through_elementwise(t):      # follow a conv's output through bn / relu to what the next layer reads
        while any(c["kind"] in ("bn", "same") for c in consumers.get(t, [])):
            t = next(c["dst"] for c in consumers[t] if c["kind"] in ("bn", "same"))
        return t

    layers = []
    for e in ev:
        if e["kind"] != "conv":
            continue
        out = through_elementwise(e["dst"])
        layers.append(Layer(e["name"], e["cin"], e["cout"], e["ks"], e["pad"], e["hin"], e["win"], e["ho"], e["wo"],
                            ups=int(produced.get(e["src"], {}).get("kind") == "up"),
                            pool=int(any(c["kind"] == "pool" for c in consumers.get(out, []))),
                            bn=any(c["kind"] == "bn" for c in consumers.get(e["dst"], []))))
    return layers


def gflop_per_frame(h: int, w: int, patches: float, n_ids: int = 16) -> float:
    """Every conv2d of both networks as written: the figure DESIGN.md 5 quotes."""
    det = sum(l.flops for l in trace_layers("detector", h, w, n_ids))
    ref = sum(l.flops for l in trace_layers("refinenet", 24, 24))
    return (det + patches * ref) / 1e9


@dataclass(frozen=True)
class Rec:
    """One expected record.  ``kernel_id``: the bracket's id, None for a convolution launch, whose instantiation is whatever
    ``dcx_conv_pick_name_ups(*pick)`` names.  ``layers``: the oracle layers the launch computes."""
    layers: Tuple[str, ...]
    kernel_id: Optional[int]
    n: int
    limited: int
    flops: int
    pick: Optional[Tuple[int, ...]] = None     # (n, cin, ho, wo, cout, ks, pool, epi, ups)


def _by_name(layers):
    return {l.name: l for l in layers}


def _conv(l: Layer, n: int, limited: int, pick_n: int, epi: int = EPI_BNRELU, cout: Optional[int] = None, flops: Optional[int] = None,
          names: Optional[Tuple[str, ...]] = None, flat: bool = False) -> Rec:
    cout = l.cout if cout is None else cout
    ho, wo = (1, l.ho * l.wo) if flat else (l.ho, l.wo)      # 1x1 layers: the image flattened to 1 x cells
    return Rec(names or (l.name,), None, n, limited, l.flops if flops is None else flops,
               (pick_n, l.cin, ho, wo, cout, l.ks, l.pool, epi, l.ups))


def _detector_body(h, w, batch, n_ids):
    """conv1b .. conv4b, then convPa|convDa as one launch of 512 couts (both read conv4b's output)."""
    L = _by_name(trace_layers("detector", h, w, n_ids))
    assert list(L) == ["conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPa", "convPb", "convDa", "convDb"]
    recs = [Rec(("conv1a",), PROF_CONV1A, batch, 0, 0)]
    recs += [_conv(L[k], batch, 0, batch) for k in ("conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b")]
    pa, da = L["convPa"], L["convDa"]
    assert (pa.cin, pa.ks, pa.ho, pa.wo, pa.pool, pa.ups) == (da.cin, da.ks, da.ho, da.wo, da.pool, da.ups)
    recs.append(_conv(pa, batch, 0, batch, cout=pa.cout + da.cout, flops=pa.flops + da.flops, names=("convPa", "convDa")))
    return L, recs


def _refiner(p, limited, pick_n):
    """101, conv1b .. conv5b, convPa (+ convPb and the tile arg-max in its epilogue, not counted), 103."""
    L = _by_name(trace_layers("refinenet", 24, 24))
    assert list(L) == ["conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "conv5a", "conv5b", "convPa", "convPb"]
    recs = [Rec(("conv1a",), PROF_PATCHES, p, limited, 0)]
    recs += [_conv(L[k], p, limited, pick_n) for k in ("conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "conv5a", "conv5b")]
    recs.append(_conv(L["convPa"], p, limited, HEAT_PICK_N, epi=EPI_HEAT, names=("convPa", "convPb")))
    recs.append(Rec((), PROF_FINALIZE, p, limited, 0))
    return recs


def expected_infer_batch(batch: int, h: int, w: int, pool: int, n_ids: int = 16, refine: bool = True) -> List[Rec]:
    """dcx_infer_batch: the detector's 1x1 heads run inside the tail (id 102); RefineNet's grid covers the whole pool and takes the
    device-side corner count; its tiles are chosen for the expected batch * n_ids live patches where the pool is larger."""
    _, recs = _detector_body(h, w, batch, n_ids)
    recs.append(Rec(("convPb", "convDb"), PROF_TAIL, batch, 0, 0))
    if refine:
        recs += _refiner(pool, 1, min(batch * n_ids, pool))
    return recs


def expected_detector_forward(batch: int, h: int, w: int, n_ids: int = 16) -> List[Rec]:
    """dcx_detector_forward: the two raw 1x1 heads are convolution launches of their own."""
    L, recs = _detector_body(h, w, batch, n_ids)
    assert not L["convPb"].bn and not L["convDb"].bn
    recs += [_conv(L[k], batch, 0, batch, epi=EPI_RAW, flat=True) for k in ("convPb", "convDb")]
    return recs


def expected_refiner_forward(max_patches: int, with_total: bool) -> List[Rec]:
    return _refiner(max_patches, int(with_total), max_patches)


def unrecorded_flops(h: int, w: int, patches: float, n_ids: int = 16) -> float:
    """The layers no record's flops carry in dcx_infer_batch: both conv1a, the detector's 1x1 heads, RefineNet's convPb."""
    d, r = _by_name(trace_layers("detector", h, w, n_ids)), _by_name(trace_layers("refinenet", 24, 24))
    return d["conv1a"].flops + d["convPb"].flops + d["convDb"].flops + patches * (r["conv1a"].flops + r["convPb"].flops)
