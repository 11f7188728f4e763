"""The memory contract of dcx_rig_uncertainty_pool (include/deepcharuco_amd.h), on tests/guarded.py arenas
through the harness of tests/test_gpu_workspace_contract.py (its ``drive``: exact-size workspace and outputs between guards;
workspace bodies of zeros, another call's leftovers, 0x7F and 0xFF; the same bits as the call on roomy buffers each time; guards
intact), DCX_E_WS for a workspace one byte short, and the inputs (the pools, d_pose, d_view_status, the masks) left as they were.
The entry is fed what the rig calibration wrote on the device; the scenes leave a view to a failed check, a timestamp without
camera 0 and one with a single usable view, so every reduction runs over views and timestamps whose workspace parts nobody wrote.
Two cameras and eight; the leftovers are those of the call with the OTHER number of cameras, whose strides differ."""
import ctypes

import numpy as np
import pytest
import torch

import rig_exact as rx
from deepcharuco_amd import _lib, calib, pnp, rig
from test_gpu_rig import CAMS8, _hand_built_pool, _table
from test_gpu_rig_cov import _compare
from test_gpu_workspace_contract import F64, FSENT, _gpu, _stream, drive
from test_rig_cov_host import SIGMA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


class Solved:
    """C hand-built pools on the device, calibrated there: what the uncertainty entry is handed."""

    def __init__(self, dev, n_cams, seed, n_stamps):
        C = self.C = n_cams
        spec = dict(angles=(0, 30), cams=("A", "B")) if C == 2 else CAMS8
        vis = np.ones((n_stamps, C), bool)
        vis[2, 0] = False                                              # a timestamp without camera 0 (C = 2: one usable view)
        s = rx.scene(seed, n_stamps, visible=vis, sigma=SIGMA, rows=10, **spec)
        kps = [[k.copy() for k in kl] for kl in s.kps]
        kps[1][4] = kps[1][4][:3]                                      # TOO_FEW
        if C > 2:
            kps[2][1][0, 2] = -1                                       # BAD_ID
        self.s, self.kps, self.B = s, kps, n_stamps
        self.cameras, self.dists = rx.cam_args(s)
        self.pools = [2 + sum(len(k) + 3 for k in kps[c]) + 5 for c in range(C)]
        self.packed = [_gpu(dev, _hand_built_pool(kps[c], self.pools[c], seed + c)) for c in range(C)]
        rng = np.random.default_rng(seed)
        self.masks = [_gpu(dev, (rng.random(p) < 0.9).astype(np.uint8)) if c % 2 else None for c, p in enumerate(self.pools)]
        r = self.r = rig.rig_calibrate_pools(self.packed, self.B, self.pools, True, *s.board, self.cameras, self.dists, masks=self.masks)
        assert r.status == rig.RIG_OK
        self.st = _gpu(dev, r.view_status.astype(np.int32))
        pose = np.zeros((self.B, 8))
        pose[:, :6] = np.c_[r.rvecs, r.tvecs]
        self.pose = _gpu(dev, pose)
        self.table = _table(self.packed, self.B, self.pools, self.cameras, self.dists, self.masks)
        self.x = (ctypes.c_double * (6 * (C - 1)))(*np.c_[r.rvec, r.T][1:].ravel().tolist())
        self.hp = (ctypes.c_int * C)(*self.pools)

    def call(self, L, ws_ptr, nbytes, g_ptr, p_ptr):
        return L.dcx_rig_uncertainty_pool(self.C, self.table, None, self.x, self.B, *self.s.board, self.st.data_ptr(),
                                          self.pose.data_ptr(), ws_ptr, nbytes, g_ptr, p_ptr, _stream())


@pytest.mark.parametrize("n_cams", [2, 8])
def test_rig_uncertainty_pool(dev, L, n_cams):
    a = Solved(dev, n_cams, 81, 9)
    other = Solved(dev, 10 - n_cams, 82, 9 if n_cams == 2 else 140)    # the leftovers come from the larger workspace
    need, need2 = L.dcx_rig_uncertainty_workspace_bytes(a.C, a.B, a.hp), L.dcx_rig_uncertainty_workspace_bytes(other.C, other.B, other.hp)
    assert 0 < need < need2
    inputs = {"pools": [p.clone() for p in a.packed], "st": a.st.clone(), "pose": a.pose.clone(),
              "masks": [None if m is None else m.clone() for m in a.masks]}
    n = 6 * (a.C - 1)

    def setup(bufs):
        ws = bufs.workspace("ws", need, need2, align=8)
        g = bufs.output("global", (rig.RIGCOV_GLOBAL_WORDS,), F64, FSENT)
        p = bufs.output("pose_cov", (a.B, calib.COV_POSE_WORDS), F64, FSENT)

        def run():
            assert a.call(L, ws.ptr, need - 1, g.ptr, p.ptr) == -3                                # DCX_E_WS
            assert a.call(L, ws.ptr, need, g.ptr, p.ptr) == 0
            return {"global": g.cpu().copy(), "pose_cov": p.cpu().copy()}
        return run

    def left(bufs):
        tmp = torch.zeros(rig.RIGCOV_GLOBAL_WORDS + other.B * calib.COV_POSE_WORDS, dtype=F64, device=bufs.dev)
        assert other.call(L, bufs.ws["ws"].ptr, need2, tmp.data_ptr(), tmp[rig.RIGCOV_GLOBAL_WORDS:].data_ptr()) == 0
        torch.cuda.synchronize()
        assert int(tmp[rig.RIGCOV_SIGMA2 + 4]) == calib.COV_OK and int(tmp[rig.RIGCOV_SIGMA2 + 3]) == other.r.stamps_used

    def after(g, got):
        used = (a.r.view_status == pnp.PNP_OK).sum(1) >= 2
        assert not got["pose_cov"][~used].any() and got["pose_cov"][used].all()
        cov = got["global"][:rig.RIGCOV_STD].reshape(42, 42)
        assert not cov[n:].any() and not cov[:, n:].any() and not got["global"][rig.RIGCOV_STD + n:rig.RIGCOV_SIGMA2].any()
        assert got["global"][rig.RIGCOV_GLOBAL_WORDS - 1] == 0.0
        assert all(torch.equal(p, q) for p, q in zip(a.packed, inputs["pools"])) and torch.equal(a.st, inputs["st"])
        assert all(m is None or torch.equal(m, q) for m, q in zip(a.masks, inputs["masks"]))
        assert a.pose.cpu().numpy().tobytes() == inputs["pose"].cpu().numpy().tobytes()
        return {"status": int(got["global"][rig.RIGCOV_SIGMA2 + 4])}

    want, _ = drive(f"rig_uncertainty_pool/{n_cams} cameras", dev, setup, left, after=after)
    d = rig.unpack_rig_uncertainty(torch.from_numpy(want["global"]), torch.from_numpy(want["pose_cov"]), a.r.T)
    assert d.status == calib.COV_OK and d.stamps == a.r.stamps_used and d.points == a.r.points_used
    # the definition at the device's solution, on the rows the masks keep: a pool holds a view's rows id-sorted
    masks = []
    for c in range(a.C):
        if a.masks[c] is None:
            masks.append(None)
            continue
        m = a.masks[c].cpu().numpy().astype(bool)
        packed = a.packed[c].cpu().numpy()
        counts, starts = packed[:a.B], packed[a.B:2 * a.B]
        per = []
        for t, kp in enumerate(a.kps[c]):
            by_slot = m[starts[t]:starts[t] + counts[t]]
            per.append(by_slot[np.argsort(np.argsort(kp[:, 2], kind="stable"), kind="stable")])   # slot order -> the list's
        masks.append(per)
    _compare(d, rig.rig_uncertainty_host(a.kps, *a.s.board, a.cameras, a.dists, a.r, masks=masks),
             f"rig_uncertainty_pool on guarded buffers, {n_cams} cameras")
