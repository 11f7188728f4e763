"""CPU: the C-ABI surface of the two-call batch path (dcx_detector_front, dcx_infer_batch_prefetched, dcx_front_bytes):
declared in the header, in the ctypes table and in the library, and refusing bad arguments before any device call."""
import ctypes
import os
import re

from conftest import REPO

NEW = ("dcx_front_bytes", "dcx_detector_front", "dcx_infer_batch_prefetched")


def test_prefetch_exports_are_declared_everywhere():
    from deepcharuco_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(REPO, "include", "deepcharuco_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(dcx_[a-z0-9_]+)\s*\(", header))
    table = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(handle, name)
        assert f"`{name}`" in table
    # the prefetched entry takes dcx_infer_batch's arguments plus the set and its size behind the workspace and the event in front of the stream
    a, b = _lib.SIGNATURES["dcx_infer_batch"][1], _lib.SIGNATURES["dcx_infer_batch_prefetched"][1]
    assert b[:13] == a[:13] and b[13:15] == [ctypes.c_void_p, ctypes.c_size_t] and b[15:20] == a[13:18] and b[20:] == [ctypes.c_void_p] * 2


def test_prefetch_entries_reject_bad_arguments_without_a_gpu():
    from deepcharuco_amd import _lib
    lib = _lib.lib()
    E_ARG, E_SHAPE, E_NIDS = -1, -2, -4
    # never dereferenced: every call below fails its checks first
    fake = ctypes.create_string_buffer(4096)
    p = ctypes.cast(fake, ctypes.c_void_p)
    assert lib.dcx_front_bytes(None, 3, 64, 96) == 0
    assert lib.dcx_front_bytes(p, 0, 64, 96) == 0 and lib.dcx_front_bytes(p, 3, 64, 0) == 0
    assert lib.dcx_front_bytes(p, 3, 64, 96) >= 3 * 64 * 64 * 96 * 4 + (64 + 3) * 4

    def front(det=p, frames=p, pitch=96, pix=0, b=3, h=64, w=96, fs=p, nb=1 << 30):
        return lib.dcx_detector_front(det, frames, h * pitch, pitch, pix, b, h, w, fs, nb, None)
    assert front(det=None) == E_ARG and front(frames=None) == E_ARG and front(fs=None) == E_ARG
    assert front(pix=3) == E_ARG
    assert front(b=0) == E_SHAPE and front(h=7) == E_SHAPE and front(w=7) == E_SHAPE
    assert front(pitch=95) == E_SHAPE and front(pix=1, pitch=3 * 96 - 1) == E_SHAPE
    assert front(nb=16) == -3

    def rest(det=p, rf=p, frames=p, pitch=96, pix=0, b=3, h=64, w=96, dust=16, pool=192, ws=p, fs=p, nb=1 << 30, counts=p,
             starts=p, rows=p, xy=p):
        return lib.dcx_infer_batch_prefetched(det, rf, frames, h * pitch, pitch, pix, b, h, w, dust, pool, ws, 1 << 30, fs, nb,
                                              counts, starts, rows, xy, None, None, None)
    for name in ("det", "frames", "ws", "fs", "counts", "starts", "rows", "xy"):
        assert rest(**{name: None}) == E_ARG, name
    assert rest(pix=-1) == E_ARG
    assert rest(pool=0) == E_SHAPE and rest(pool=(1 << 22) + 1) == E_SHAPE
    assert rest(b=0) == E_SHAPE and rest(h=4) == E_SHAPE and rest(pitch=10) == E_SHAPE
    assert rest(dust=256) == E_NIDS and rest(dust=-1) == E_NIDS
    assert rest(nb=16) == -3
