"""Shared plumbing for the model mirrors: device checks, ownership of the native weights, workspace cache."""
from __future__ import annotations

import ctypes as C
import sys
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from ..weights import StateDict, state_dict_keys, validate_state_dict


_cuda_checked: dict = {}       # device argument -> resolved device, for arguments that name an index (a per-call cost on the one-frame path)


def require_cuda(device) -> torch.device:
    try:
        hit = _cuda_checked.get(device)
    except TypeError:           # unhashable argument: the slow path decides
        hit = None
    if hit is not None:
        return hit
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(
            f"deepcharuco_amd runs on MI355X (device 'cuda'); got device={device!r}. "
            "There is no CPU fallback -- use the reference implementation on CPU.")
    if not torch.cuda.is_available():
        raise RuntimeError("deepcharuco_amd needs a visible ROCm GPU (torch.cuda.is_available() is False)")
    if dev.index is None:
        return torch.device("cuda", torch.cuda.current_device())      # follows the current device: not memoised
    try:
        _cuda_checked[device] = dev
    except TypeError:
        pass
    return dev


def tensor_pointer_array(sd: StateDict, kind: str, n_ids: int):
    """Host float32 arrays in state_dict_keys() order -> (ctypes void* array, keep-alive list)."""
    validate_state_dict(sd, kind, n_ids)
    keep = [np.ascontiguousarray(sd[k], dtype=np.float32) for k in state_dict_keys(kind, n_ids)]
    arr = (C.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
    return arr, keep


class Workspace:
    """Grow-only device scratch buffers (torch uint8 tensors), one per (tag, device, HIP stream).

    Owned by a model object, keyed by the stream that is current when it is requested: two streams (or two threads on
    two streams) driving the same model never share activations, and a buffer is only ever used -- and, when it has to
    grow, released -- on the stream it was allocated on, so torch's stream-ordered allocator keeps the old block alive
    until the kernels already queued on that stream are done with it."""

    def __init__(self):
        self._buf: Dict[Tuple[str, int, int], torch.Tensor] = {}

    def get(self, tag: str, device: torch.device, nbytes: int) -> torch.Tensor:
        key = (tag, device.index, torch.cuda.current_stream(device).cuda_stream)
        buf = self._buf.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = None
            self._buf.pop(key, None)
            buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
            self._buf[key] = buf
        return buf


def check_dev_tensor(t: torch.Tensor, device: torch.device, dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); deepcharuco_amd has no CPU path")
    if device is not None and device.index is not None and t.device != device:
        raise RuntimeError(f"{name} lives on {t.device} but the model's weights are on {device}")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def unwrap(model):
    """The inner model of a Lightning-style wrapper (``lModel`` / ``lRefineNet``, or anything with ``.model``), else the argument
    (None included)."""
    return model.model if hasattr(model, "model") else model


class NativeWeights:
    """One native weight set (a ``dcx_detector`` / ``dcx_refiner`` handle, its device, its destroy function), destroyed exactly once:
    by ``free()`` or with the last reference.  The model holds its current weights and every hipGraph captured with them holds them
    too (graph.GraphedPipeline), so a reload frees weights a graph may still replay only once that graph is gone."""

    def __init__(self, handle: C.c_void_p, device: torch.device, destroy: Callable[[C.c_void_p], int]):
        self.handle: Optional[C.c_void_p] = handle
        self.device = device
        self._destroy = destroy

    def free(self) -> None:
        h, self.handle = self.handle, None
        if h is not None:
            self._destroy(h)

    def __del__(self):
        try:
            self.free()
        except Exception:           # interpreter shutdown: the library may already be unloaded
            pass


class NativeModel:
    """Base of ``dcModel`` / ``RefineNet``: weights, device, source state dict and scratch buffers; a subclass supplies ``_create``."""

    _kind = ""                          # weights.state_dict_keys kind

    def __init__(self, state_dict: Optional[StateDict] = None, device="cuda"):
        self._weights: Optional[NativeWeights] = None
        self._device: Optional[torch.device] = None
        self._ws = Workspace()
        self._sd = None
        if state_dict is not None:
            self.load_state_dict(state_dict, device)

    def _create(self, arr, n_tensors: int) -> Tuple[C.c_void_p, Callable[[C.c_void_p], int]]:
        raise NotImplementedError       # dcx_*_create on the current device -> (handle, its destroy function)

    def load_state_dict(self, state_dict: StateDict, device="cuda"):
        dev = require_cuda(device)
        arr, keep = tensor_pointer_array(state_dict, self._kind, getattr(self, "n_ids", 16))     # (only the detector has n_ids)
        self._release()
        with torch.cuda.device(dev):
            h, destroy = self._create(arr, len(keep))
        self._weights = NativeWeights(h, dev, destroy)
        self._device, self._sd = dev, state_dict
        return self

    def to(self, device):
        dev = require_cuda(device)
        if self._sd is not None and dev != self._device:
            self.load_state_dict(self._sd, dev)
        return self

    def eval(self):                     # BN is always evaluated with running statistics (inference.py:75)
        return self

    @property
    def handle(self) -> C.c_void_p:
        if self._weights is None:
            raise RuntimeError(f"{type(self).__name__} has no weights loaded (call load_state_dict / load_models)")
        return self._weights.handle

    @property
    def device(self) -> torch.device:
        if self._device is None:
            raise RuntimeError(f"{type(self).__name__} has no weights loaded")
        return self._device

    def _release(self):
        """Retire the hipGraphs captured with the weights, then drop this model's reference: weights no graph holds die here."""
        w, g = self._weights, sys.modules.get("deepcharuco_amd.graph")      # (no import: __del__ may run at interpreter shutdown)
        try:
            if w is not None and g is not None:
                g.drop_graphs_of(w)
        finally:
            self._weights = w = None    # (w too: a traceback must not keep them alive)

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


class NativeWrapper:
    """Base of the Lightning-wrapper mirrors ``lModel`` / ``lRefineNet``: the calls they forward to their ``.model``."""

    def forward(self, x):
        return self.model(x)

    __call__ = forward

    def eval(self):
        self.model.eval()
        return self

    def to(self, device):               # always reloads (the inner model's ``to`` only when the device changes)
        if self.model._sd is None:
            raise RuntimeError("no weights loaded")
        self.model.load_state_dict(self.model._sd, device)
        return self
