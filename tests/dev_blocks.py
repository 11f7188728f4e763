"""ctypes wrapper of tests/csrc/dev_blocks.hip: the fp64 device building blocks of deepcharuco_amd/csrc, each behind one thin kernel
(test infrastructure only).  One Python call per block takes and returns numpy arrays; the arrays travel through torch tensors on
the current device and the kernels run on torch's current stream, so a call can be captured in a graph.

The harness pins the source text of the blocks (dcx_mat_dev.h, dcx_camera_dev.h, dcx_fisheye_dev.h, dcx_pnp_dev.h), compiled with the
library's own flags.  It does not pin the instructions inside the library's kernels, which are another compilation of the same text:
those stay pinned end to end by the solver tests."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc")
_LIB_SRC = os.path.join(os.path.dirname(_HERE), "deepcharuco_amd", "csrc")
_PATH = os.path.join(_HERE, "libdcx_dev_blocks.so")
_lib = None

LANES = 64
# what a launcher's outputs hold before it runs: a NaN with a payload of its own, and an int no block returns
FILL_BITS = 0x7FF8DEAD0000BEEF
FILL = np.array([FILL_BITS], np.uint64).view(np.float64)[0]
IFILL = -777777

# name -> (lanes per instance, NIN, NIIN, NOUT, NIOUT): the LANE(...) and WAVE(...) blocks of dev_blocks.hip
BLOCKS = {
    "rodrigues": (1, 3, 1, 9, 1), "rvec_of": (1, 9, 1, 3, 1), "right_jacobian": (1, 3, 1, 9, 1), "pose_basis": (1, 3, 1, 27, 1),
    "pose_columns": (1, 26, 1, 12, 1), "distort": (1, 10, 1, 5, 1), "project": (1, 17, 1, 12, 1), "project_nojac": (1, 17, 1, 2, 1),
    "undistort": (1, 14, 1, 2, 1), "fisheye_distort": (1, 6, 1, 7, 1), "fisheye_project": (1, 13, 1, 14, 1),
    "fisheye_project_nojac": (1, 13, 1, 2, 1), "fisheye_undistort": (1, 10, 1, 2, 1), "jacobi3": (1, 6, 1, 15, 1),
    "polar_factor": (1, 9, 1, 9, 1), "cholesky_factor": (1, 22, 1, 21, 1), "cholesky_substitute": (1, 27, 1, 6, 1),
    "cholesky_solve": (1, 28, 1, 6, 1), "adjugate": (1, 9, 1, 9, 1), "projective_basis": (1, 8, 1, 9, 1),
    "homography4": (1, 16, 1, 11, 1), "init_pose4": (1, 16, 1, 6, 1), "mix32": (1, 1, 1, 1, 1), "ransac_draw": (1, 1, 4, 1, 1),
    "on_a_line": (1, 1, 11, 1, 1), "unpk": (1, 1, 1, 1, 12), "pk": (1, 1, 2, 1, 6),
    "wave_sum5": (LANES, 64 * 5, 1, 5, 1), "wave_sum28": (LANES, 64 * 28, 1, 28, 1), "append_kept": (LANES, 1, 65, 1, 2),
    "jacobi9": (LANES, 45, 1, 54, 1),
}
UNPK_N = (6, 8, 9, 13, 15, 16)           # the N of unpk / pk in use: U, theta (fisheye, pinhole), stereo rows, calibration rows


def sources():
    return [os.path.join(_SRC, "dev_blocks.hip"), os.path.join(_SRC, "Makefile")] + sorted(glob.glob(os.path.join(_LIB_SRC, "*.h")))


def build():
    r = subprocess.run(["make", "-C", _SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("building tests/libdcx_dev_blocks.so failed:\n" + r.stdout)
    return _PATH


def stale():
    return not os.path.exists(_PATH) or os.path.getmtime(_PATH) < max(os.path.getmtime(s) for s in sources())


def lib():
    global _lib
    if _lib is None:
        if stale():
            build()
        h = C.CDLL(_PATH)
        P, I = C.c_void_p, C.c_int
        for name in BLOCKS:
            getattr(h, "dcxt_" + name).argtypes = [P, P, P, P, I, P]
        h.dcxt_ransac_sample.argtypes = [P, I, P, P, I, P]
        h.dcxt_best_hypothesis.argtypes = [P, I, P, P, I, P]
        h.dcxt_block_tree6.argtypes = h.dcxt_block_tree7.argtypes = [P, P, I, P]
        h.dcxt_accumulate_rows.argtypes = [P, P, I, P, P, P, P, I, P]
        for na in (6, 8, 9):
            getattr(h, f"dcxt_schur_view{na}").argtypes = [P, P, P, P, P, I, P]
        pool = [P, P, P, P, I, I, I, I, C.c_double]
        h.dcxt_frame_checks.argtypes = pool + [P, P]
        h.dcxt_frame_blocks_pinhole.argtypes = h.dcxt_frame_blocks_fisheye.argtypes = pool + [P, P, P, P, P]
        _lib = h
    return _lib


# ------------------------------------------------------------------------------------------------ device arrays

def _torch():
    import torch
    return torch


def to_dev(a, dtype):
    torch = _torch()
    a = np.ascontiguousarray(a, dtype)
    if a.size == 0:
        a = np.zeros(1, dtype)
    return torch.from_numpy(a.copy()).cuda()


def filled(count, dtype):
    """A device array of ``count`` fill values (FILL for float64, IFILL for int32)."""
    if dtype == np.float64:
        return to_dev(np.full(max(count, 1), FILL_BITS, np.uint64).view(np.float64), np.float64)
    return to_dev(np.full(max(count, 1), IFILL, np.int32), np.int32)


def _stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def untouched(a):
    """Which float64 entries still hold the fill, by their bits."""
    return np.ascontiguousarray(a, np.float64).view(np.uint64) == FILL_BITS


def launch(name, d_in, d_iin, d_out, d_iout, n):
    """The raw launcher on device tensors (for graph capture) -> its return code."""
    return getattr(lib(), "dcxt_" + name)(_p(d_in), _p(d_iin), _p(d_out), _p(d_iout), int(n), _stream())


def run(name, x=None, ix=None, n=None):
    """Block ``name`` on n instances: x (n, NIN) float64 and / or ix (n, NIIN) int32 -> (out, iout).  Per-lane blocks give
    (n, NOUT) and (n, NIOUT); wave-wide ones (n, 64, NOUT) and (n, 64, NIOUT), one row per lane."""
    torch = _torch()
    lanes, nin, niin, nout, niout = BLOCKS[name]
    if n is None:
        n = len(x) if x is not None else len(ix)
    x = np.zeros((n, nin)) if x is None else np.ascontiguousarray(x, np.float64).reshape(n, nin)
    ix = np.zeros((n, niin), np.int32) if ix is None else np.ascontiguousarray(ix).astype(np.int32).reshape(n, niin)
    d_in, d_iin = to_dev(x, np.float64), to_dev(ix, np.int32)
    d_out, d_iout = filled(n * lanes * nout, np.float64), filled(n * lanes * niout, np.int32)
    rc = launch(name, d_in, d_iin, d_out, d_iout, n)
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    shape = (n,) if lanes == 1 else (n, lanes)
    return d_out.cpu().numpy().reshape(shape + (nout,)), d_iout.cpu().numpy().reshape(shape + (niout,))


def ransac_sample(ids, cases):
    """ids: the id of every slot of one frame; cases (m, 4) = seed, n, h, rm1 -> (m, 5) = ok, s0..s3 (ok = -1: not run)."""
    torch = _torch()
    rows = np.zeros((len(ids), 4), np.int32)
    rows[:, 2] = ids
    cases = np.ascontiguousarray(cases).astype(np.int64).astype(np.uint32).view(np.int32).reshape(-1, 4)
    d_rows, d_c, d_o = to_dev(rows, np.int32), to_dev(cases, np.int32), filled(5 * len(cases), np.int32)
    rc = lib().dcxt_ransac_sample(_p(d_rows), len(ids), _p(d_c), _p(d_o), len(cases), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return d_o.cpu().numpy().reshape(-1, 5)


def best_hypothesis(scores, iterations):
    """scores (m, stride) int32, iterations (m,) -> (m, 64, 2) = best, bh per lane."""
    torch = _torch()
    scores = np.ascontiguousarray(scores, np.int32)
    m, stride = scores.shape
    d_s, d_i, d_o = to_dev(scores, np.int32), to_dev(iterations, np.int32), filled(m * LANES * 2, np.int32)
    rc = lib().dcxt_best_hypothesis(_p(d_s), stride, _p(d_i), _p(d_o), m, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return d_o.cpu().numpy().reshape(m, LANES, 2)


def block_tree_threads():
    return lib().dcxt_block_tree_threads()


def block_tree(x):
    """x (m, THREADS, NV), NV = 6 or 7 -> (m, NV) totals."""
    torch = _torch()
    x = np.ascontiguousarray(x, np.float64)
    m, t, nv = x.shape
    assert t == block_tree_threads() and nv in (6, 7)
    d_x, d_o = to_dev(x, np.float64), filled(m * nv, np.float64)
    rc = getattr(lib(), f"dcxt_block_tree{nv}")(_p(d_x), _p(d_o), m, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return d_o.cpu().numpy().reshape(m, nv)


def accumulate_rows(rows, front, counts, starts):
    """rows (R, 2, 13), front (R,), instance b owns rows starts[b] : starts[b] + counts[b]
    -> acc (m, 64, 2), (ea, eb) (m, 64, 2) each, behind (m, 64)."""
    torch = _torch()
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 26)
    m = len(counts)
    d = [to_dev(rows, np.float64), to_dev(front, np.int32), to_dev(counts, np.int32), to_dev(starts, np.int32)]
    d_o, d_io = filled(m * LANES * 2, np.float64), filled(m * LANES * 5, np.int32)
    rc = lib().dcxt_accumulate_rows(_p(d[0]), _p(d[1]), len(rows), _p(d[2]), _p(d[3]), _p(d_o), _p(d_io), m, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    io = d_io.cpu().numpy().reshape(m, LANES, 5)
    return d_o.cpu().numpy().reshape(m, LANES, 2), io[:, :, 0:2], io[:, :, 2:4], io[:, :, 4]


def schur_view(na, m, scale):
    """m (B, packed (na + 7)^2), scale (B,) -> sc (B, NS + na), yz (B, 6 na + 6), verdict (B, 64)."""
    torch = _torch()
    m = np.ascontiguousarray(m, np.float64)
    B = len(m)
    nc = na + 7
    assert m.shape[1] == nc * (nc + 1) // 2
    ksc, kyz = na * (na + 1) // 2 + na, 6 * na + 6
    d_m, d_s = to_dev(m, np.float64), to_dev(scale, np.float64)
    d_sc, d_yz, d_io = filled(B * ksc, np.float64), filled(B * kyz, np.float64), filled(B * LANES, np.int32)
    rc = getattr(lib(), f"dcxt_schur_view{na}")(_p(d_m), _p(d_s), _p(d_sc), _p(d_yz), _p(d_io), B, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return d_sc.cpu().numpy().reshape(B, ksc), d_yz.cpu().numpy().reshape(B, kyz), d_io.cpu().numpy().reshape(B, LANES)


def _pool_dev(counts, starts, rows, xy):
    xy_d = None if xy is None else to_dev(xy, np.float32)
    return to_dev(counts, np.int32), to_dev(starts, np.int32), to_dev(rows, np.int32), xy_d


def frame_checks(counts, starts, rows, xy, pool, board):
    """frame_status and ranges_overlap on every frame of a pool -> (B, 64, 4) = status, n, s0, overlap per lane."""
    torch = _torch()
    B = len(counts)
    c, s, r, x = _pool_dev(counts, starts, rows, xy)
    d_io = filled(B * LANES * 4, np.int32)
    rc = lib().dcxt_frame_checks(_p(c), _p(s), _p(r), None if x is None else _p(x), B, int(pool), int(board[0]), int(board[1]),
                                 float(board[2]), _p(d_io), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return d_io.cpu().numpy().reshape(B, LANES, 4)


FRAME_OUT = {"acc": slice(0, 28), "cost": 28, "H": slice(29, 38), "mc": slice(38, 40), "p0": slice(40, 46), "pose": slice(46, 54)}
FRAME_IOUT = {"readable": 0, "st_H": 1, "st_init": 2, "st_solve": 3, "inside": 4}


def frame_blocks(model, counts, starts, rows, xy, pool, board, camera, poses):
    """evaluate<true>, evaluate<false>, points_inside, homography, init_pose and solve on every frame of a pool, frame b at pose
    poses[b]; camera = fx fy cx cy + 8 (pinhole) or 4 (fisheye) coefficients -> out (B, 64, 54) by FRAME_OUT, iout (B, 64, 5) by
    FRAME_IOUT."""
    torch = _torch()
    B = len(counts)
    c, s, r, x = _pool_dev(counts, starts, rows, xy)
    cam = np.zeros(12)
    cam[:len(camera)] = camera
    d_cam, d_p = to_dev(cam, np.float64), to_dev(np.asarray(poses, np.float64).reshape(B, 6), np.float64)
    d_o, d_io = filled(B * LANES * 54, np.float64), filled(B * LANES * 5, np.int32)
    rc = getattr(lib(), "dcxt_frame_blocks_" + model)(_p(c), _p(s), _p(r), None if x is None else _p(x), B, int(pool), int(board[0]),
                                                      int(board[1]), float(board[2]), _p(d_cam), _p(d_p), _p(d_o), _p(d_io), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return d_o.cpu().numpy().reshape(B, LANES, 54), d_io.cpu().numpy().reshape(B, LANES, 5)
