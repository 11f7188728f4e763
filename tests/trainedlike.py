"""Loader of the trained-regime golden cases (tests/golden/trainedlike_*.npz, oracle/make_golden.py).

Their detector weights carry a shifted no-corner bias (``convPb.bias[64]``): class 64 wins on 85-95 % of the cells, as with trained
checkpoints, so the ``where(loc_argmax == 64, dust_bin_ids, ids_argmax)`` rule of ``pred_argmax`` (models/model_utils.py:76) hides
the ids head on most cells.  ``GoldenCase`` (conftest.py) checks the weights' SHA before any loc-bias could be applied, so these
cases have a loader of their own: the same steps, plus ``convPb.bias`` from the fixture, then the same strict SHA check on the
final state dict."""
import json
import os

import numpy as np

from conftest import GOLDEN, GoldenCase

TRAINED_CASES = ["trainedlike_board_240x320", "trainedlike_img7412_240x320", "trainedlike_board_480x640"]
MIN_MASKED_CELLS = 20     # oracle/make_golden.py asserts the same on the reference's own pred_argmax


class TrainedLikeCase(GoldenCase):
    def __init__(self, name):
        from deepcharuco_amd import weights as W
        self.name = name
        self.fx = np.load(os.path.join(GOLDEN, f"{name}.npz"))
        self.meta = json.loads(str(self.fx["meta"]))
        m = self.meta
        self.n_ids = m["n_ids"]
        self.sd_dc = W.synthetic_state_dict("detector", m["wseed"], m["n_ids"])
        self.sd_dc["convPb.bias"] = self.fx["convPb_bias"].astype(np.float32).copy()
        self.sd_dc["convDb.bias"] = self.fx["convDb_bias"].astype(np.float32).copy()
        self.sd_dc["convDb.bias"][m["n_ids"]] = self.fx["dust_bias"]
        self.sd_rn = W.synthetic_state_dict("refinenet", m["wseed"] + 1)
        self._bgr = None
        if "bgr_image" in self.fx:
            from deepcharuco_amd.imgproc import bgr2gray_fixed_point
            self._bgr = np.ascontiguousarray(self.fx["bgr_image"])
            self.frame = bgr2gray_fixed_point(self._bgr)
        else:
            self.frame = W.synthetic_frames(m["kind"], m["fseed"], 1, m["H"], m["W"])[0]
        assert W.state_dict_sha256(self.sd_dc, "detector", m["n_ids"]) == str(self.fx["sha_dc"]), \
            "regenerated detector weights differ from the ones the fixture was made with"
        assert W.state_dict_sha256(self.sd_rn, "refinenet") == str(self.fx["sha_rn"])
        assert W.frames_sha256(self.frame) == str(self.fx["sha_frame"])

    def masked_cells(self):
        """Cells whose loc arg-max is the no-corner class 64 while the raw ids arg-max is not the dust bin (recomputed)."""
        fx = self.fx
        return int(((fx["loc_argmax"] == 64) & (fx["ids_argmax_raw"] != self.n_ids)).sum())


_cache = {}


def trained_case(name):
    if name not in _cache:
        _cache[name] = TrainedLikeCase(name)
    return _cache[name]
