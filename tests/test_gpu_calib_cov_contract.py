"""The memory contract of dcx_calibrate_uncertainty_pool (include/deepcharuco_amd.h), on tests/guarded.py arenas through the harness of
tests/test_gpu_workspace_contract.py (its ``drive``: exact-size workspace and outputs between guards; workspace bodies of zeros,
another call's leftovers, 0x7F and 0xFF; the same bits as the call on roomy buffers each time; guards intact), DCX_E_WS for a
workspace one byte short, and the inputs (the pool, d_pose, d_view_status, the mask) left as they were.  The entry is fed what the
calibrations wrote on the device: eight views of which three fail three different checks, so every reduction runs over views whose
workspace parts nobody wrote.  Both camera models; the leftovers are those of a 16-view call of the OTHER model's strides."""
import ctypes

import numpy as np
import pytest
import torch

import fisheye_exact as fx
from deepcharuco_amd import _lib, calib, corner_pool, fisheye as fe, pnp
from test_calib_cov_host import SIGMA
from test_calib_host import BOARD, SIZE
from test_gpu_calib_cov import _compare
from test_gpu_fisheye_contract import _pool as fisheye_pool
from test_gpu_workspace_contract import F64, FSENT, _gpu, _stream, calib_pool, calib_views, drive

pytestmark = pytest.mark.gpu

FE_K, FE_DIST = fx.camera(150.0, 152.0, off=(4.0, -3.0)), fx.K_LENS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _fisheye_views(seed, n_ok):
    """n_ok views that stand at 0.3 px, then three rows, an id outside the board, and a view cut by the pool's end."""
    _, imgs, ids_l, _ = fx.make_views(seed, n_ok + 1, FE_K, FE_DIST, sigma=SIGMA)
    kps = fx.keypoints(imgs, ids_l)
    bad = kps[1].copy()
    bad[1, 2] = 28
    return kps[:n_ok] + [kps[0][:3].copy(), bad, kps[n_ok].copy()], [pnp.PNP_OK] * n_ok + [pnp.PNP_TOO_FEW, pnp.PNP_BAD_ID,
                                                                                         pnp.PNP_TRUNCATED]


class Solved:
    """A pool on the device, calibrated there: what the uncertainty entry is handed."""

    def __init__(self, dev, L, model, seed, n_ok):
        self.model = model
        if model == calib.CAMERA_PINHOLE:
            self.views, self.expect = calib_views(seed, n_ok, sigma=SIGMA)
            packed, _, self.pool = calib_pool(self.views, seed)
            self.board, entry, extra = BOARD, L.dcx_calibrate_pool, (*SIZE,)
        else:
            self.views, self.expect = _fisheye_views(seed, n_ok)
            packed, self.pool = fisheye_pool(self.views, seed)
            self.board, entry, extra = fx.BOARD, L.dcx_fisheye_calibrate_pool, (*fx.SIZE, 0.0)
        self.B = len(self.views)
        self.packed = _gpu(dev, packed)
        self.ptrs = corner_pool.ptrs(self.packed.data_ptr(), self.B, self.pool)[:4]
        self.st = torch.empty(self.B, dtype=torch.int32, device=dev)
        self.pose = torch.empty((self.B, 8), dtype=F64, device=dev)
        need = (L.dcx_calibrate_workspace_bytes if model == calib.CAMERA_PINHOLE else L.dcx_fisheye_calibrate_workspace_bytes)(self.B)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        res = (ctypes.c_double * 16)()
        assert entry(*self.ptrs, self.B, self.pool, *self.board, *extra, ws.data_ptr(), need, self.st.data_ptr(), self.pose.data_ptr(),
                     res, _stream()) == 0
        self.res = np.array(res[:], np.float64)
        assert int(self.res[14]) == calib.CALIB_OK and int(self.res[12]) == n_ok and self.st.cpu().tolist() == self.expect
        self.ng = 9 if model == calib.CAMERA_PINHOLE else 8
        self.theta = (ctypes.c_double * 9)(*self.res[:self.ng].tolist())
        rng = np.random.default_rng(seed)
        self.mask = _gpu(dev, (rng.random(self.pool) < 0.9).astype(np.uint8))

    def call(self, L, ws_ptr, nbytes, g_ptr, p_ptr, masked=True):
        return L.dcx_calibrate_uncertainty_pool(*self.ptrs, self.B, self.pool, *self.board, self.model, self.theta, self.st.data_ptr(),
                                                self.pose.data_ptr(), self.mask.data_ptr() if masked else None, ws_ptr, nbytes,
                                                g_ptr, p_ptr, _stream())


@pytest.mark.parametrize("model", [calib.CAMERA_PINHOLE, calib.CAMERA_FISHEYE], ids=["pinhole", "fisheye"])
def test_calibrate_uncertainty_pool(dev, L, model):
    a = Solved(dev, L, model, 7, 5)
    other = Solved(dev, L, 1 - model, 8, 13)
    need, need2 = L.dcx_calibrate_uncertainty_workspace_bytes(a.B), L.dcx_calibrate_uncertainty_workspace_bytes(other.B)
    assert 0 < need < need2
    inputs = {"pool": a.packed.clone(), "st": a.st.clone(), "pose": a.pose.clone(), "mask": a.mask.clone()}

    def setup(bufs):
        ws = bufs.workspace("ws", need, need2, align=8)
        g = bufs.output("global", (calib.COV_GLOBAL_WORDS,), F64, FSENT)
        p = bufs.output("pose_cov", (a.B, calib.COV_POSE_WORDS), F64, FSENT)

        def run():
            assert a.call(L, ws.ptr, need - 1, g.ptr, p.ptr) == -3                                # DCX_E_WS
            assert a.call(L, ws.ptr, need, g.ptr, p.ptr) == 0
            return {"global": g.cpu().copy(), "pose_cov": p.cpu().copy()}
        return run

    def left(bufs):
        tmp = torch.zeros(calib.COV_GLOBAL_WORDS + other.B * calib.COV_POSE_WORDS, dtype=F64, device=bufs.dev)
        assert other.call(L, bufs.ws["ws"].ptr, need2, tmp.data_ptr(), tmp[calib.COV_GLOBAL_WORDS:].data_ptr(), masked=False) == 0
        torch.cuda.synchronize()
        assert int(tmp[94]) == calib.COV_OK and int(tmp[93]) == 13                                # thirteen views stood

    def after(g, got):
        out = np.array(a.expect) != pnp.PNP_OK
        assert not got["pose_cov"][out].any() and got["pose_cov"][~out].all()
        assert got["global"][95] == 0.0 and not got["global"][a.ng * a.ng:81].any() and not got["global"][81 + a.ng:90].any()
        assert torch.equal(a.packed, inputs["pool"]) and torch.equal(a.st, inputs["st"]) and torch.equal(a.mask, inputs["mask"])
        assert a.pose.cpu().numpy().tobytes() == inputs["pose"].cpu().numpy().tobytes()
        return {"status": int(got["global"][94])}

    want, _ = drive(f"calibrate_uncertainty_pool/{'pinhole' if model == calib.CAMERA_PINHOLE else 'fisheye'}", dev, setup, left,
                    after=after)
    d = calib.unpack_uncertainty(torch.from_numpy(want["global"]), torch.from_numpy(want["pose_cov"]), a.ng)
    assert d.status == calib.COV_OK and d.views == 5
    # the definition at the device's solution, on the rows the mask keeps
    use = [b for b in range(a.B) if a.expect[b] in (pnp.PNP_OK, pnp.PNP_TOO_FEW)]                # what the host can take
    counts, starts = corner_pool.views(a.packed.cpu().numpy(), a.B, a.pool)[:2]
    mask = a.mask.cpu().numpy().astype(bool)
    pose = a.pose.cpu().numpy()
    K = np.array([[a.res[0], 0, a.res[2]], [0, a.res[1], a.res[3]], [0, 0, 1.0]])
    host = calib.calibration_uncertainty_host if model == calib.CAMERA_PINHOLE else fe.calibration_uncertainty_fisheye_host
    # the pool holds a view's rows in the order lay_frames was given them: the views' own
    hu = host([pnp.object_points(a.views[b][:, 2], *a.board) for b in use], [a.views[b][:, :2].astype(np.float32) for b in use], K,
              a.res[4:a.ng], pose[use, :3], pose[use, 3:6], view_status=[a.expect[b] for b in use],
              inliers=[mask[starts[b]:starts[b] + counts[b]] for b in use])
    sel = np.array(use)
    _compare(d._replace(std_extrinsics=d.std_extrinsics[sel], cov_extrinsics=d.cov_extrinsics[sel]), hu,
             "calibrate_uncertainty_pool on guarded buffers", used=[use.index(b) for b in range(a.B) if a.expect[b] == pnp.PNP_OK])
