"""HIP-backed mirror of /root/reference/src/models/refinenet.py (RefineNet :9-115, lRefineNet :134-145)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from .. import _lib
from ..weights import state_dict_from_checkpoint
from ._handles import NativeModel, NativeWrapper, check_dev_tensor


class RefineNet(NativeModel):
    _kind = "refinenet"

    def _create(self, arr, n_tensors: int):
        L, h = _lib.lib(), C.c_void_p()
        _lib.check(L.dcx_refiner_create(C.byref(h), arr, n_tensors), "dcx_refiner_create")
        return h, L.dcx_refiner_destroy

    def _run(self, patches: torch.Tensor, want_heat: bool, keypoints: Optional[torch.Tensor] = None):
        dev = self.device
        patches = check_dev_tensor(patches, dev, torch.float32, "patches")
        k = patches.shape[0]
        L = _lib.lib()
        corners = torch.empty((k, 2), dtype=torch.int32, device=dev)
        heat = torch.empty((k, 1, 64, 64), dtype=torch.float32, device=dev) if want_heat else None
        xy = table = None
        if keypoints is not None:   # corners_og = (corners - 32) / 8 + keypoints computed by the finalize kernel
            if keypoints.dtype.is_floating_point or keypoints.dtype == torch.bool:
                raise TypeError("keypoints must be an integer tensor (the detector's pixel coordinates, as "
                                "pred_to_keypoints returns them); float keypoints would be truncated")
            xy = torch.empty((k, 2), dtype=torch.float32, device=dev)
            table = torch.zeros((k, 4), dtype=torch.int32, device=dev)
            table[:, 1:3] = keypoints.to(device=dev, dtype=torch.int32)
            table[:, 3] = torch.arange(k, dtype=torch.int32, device=dev)
        if k == 0:
            return corners, heat, xy
        with torch.cuda.device(dev):
            nbytes = L.dcx_refiner_workspace_bytes(self.handle, k)
            ws = self._ws.get("ref", dev, nbytes)
            _lib.check(L.dcx_refiner_forward(self.handle, patches.data_ptr(), k, None, _lib.ptr(table), ws.data_ptr(),
                                             ws.numel(), corners.data_ptr(), _lib.ptr(xy), _lib.ptr(heat),
                                             _lib.current_stream()),
                       "dcx_refiner_forward")
        return corners, heat, xy

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """refinenet.py:49-83: x (K,1,24,24) -> heat-map logits (K,1,64,64)."""
        if x.ndim != 4 or tuple(x.shape[1:]) != (1, 24, 24):
            raise ValueError(f"expected (K,1,24,24), got {tuple(x.shape)}")
        return self._run(x, True)[1]

    __call__ = forward

    def infer_patches(self, patches: torch.Tensor, keypoints: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """refinenet.py:85-115 -> (corners_og (K,2) float32, corners (K,2) int64 as (col,row))."""
        assert patches.shape[-2:] == (24, 24)
        corners32, _, corners_og = self._run(patches.reshape(-1, 24, 24), False, keypoints)
        return corners_og, corners32.to(torch.int64)


class lRefineNet(NativeWrapper):
    def __init__(self, refinenet: RefineNet):
        self.model = refinenet

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path: str, refinenet: RefineNet, map_location=None, **_):
        sd = state_dict_from_checkpoint(checkpoint_path, "refinenet")
        refinenet._sd = sd
        if map_location is not None:
            refinenet.load_state_dict(sd, map_location)
        return cls(refinenet)

    def infer_patches(self, patches, keypoints):
        return self.model.infer_patches(patches, keypoints)
