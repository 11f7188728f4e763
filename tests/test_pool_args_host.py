"""CPU: what the five entries that read the corner pool (dcx_solve_pnp_pool, dcx_solve_pnp_ransac_pool, dcx_calibrate_pool,
dcx_calibrate_ransac_pool, dcx_stereo_calibrate_pool) answer to a bad argument.  Each case starts from a valid call at batch = 1,
pool = 4 and makes one argument bad; every refusal returns before anything touches a device, so no pointer below is ever
dereferenced (and the valid call itself is never made).  EXPECTED was recorded from the library before the entries shared one
pool check (csrc/dcx_pnp_dev.h's corner_pool) and pins that behaviour, including the known asymmetry that a short workspace is
DCX_E_ARG for dcx_solve_pnp_ransac_pool and DCX_E_WS for the calibrations.
Not in the table, because they are no refusals and the call would go on to the device: dcx_solve_pnp_pool takes no workspace, and
dcx_calibrate_pool has no alignment rule for its own (a workspace misaligned by 4 is accepted there)."""
import ctypes

E_ARG, E_WS = -1, -3
BATCH, POOL, ITER = 1, 4, 100
HUGE = 46342                        # (HUGE - 1) ** 2 = 2 147 488 281 ids > 2^31 - 1

_fake = ctypes.create_string_buffer(1 << 16)
P = ctypes.cast(_fake, ctypes.c_void_p).value
assert P % 8 == 0
CAM = (ctypes.c_double * 9)(500.0, 0.0, 160.0, 0.0, 500.0, 120.0, 0.0, 0.0, 1.0)
RES = (ctypes.c_double * 16)()

POOL_PTRS = ("counts", "starts", "rows")
# entry -> (its required pointers besides the pool's, has a workspace, refuses a misaligned workspace)
ENTRIES = {
    "dcx_solve_pnp_pool": (("camera", "status", "pose"), False, False),
    "dcx_solve_pnp_ransac_pool": (("camera", "status", "pose", "info", "ws"), True, True),
    "dcx_calibrate_pool": (("ws", "status", "pose", "result"), True, False),
    "dcx_calibrate_ransac_pool": (("ws", "status", "pose", "info", "result"), True, True),
    "dcx_stereo_calibrate_pool": (("counts1", "starts1", "rows1", "ws", "status", "pose", "info", "result"), True, True),
}


def _ws_bytes(lib, entry):
    return {"dcx_solve_pnp_ransac_pool": lambda: lib.dcx_solve_pnp_ransac_workspace_bytes(BATCH, POOL, ITER),
            "dcx_calibrate_pool": lambda: lib.dcx_calibrate_workspace_bytes(BATCH),
            "dcx_calibrate_ransac_pool": lambda: lib.dcx_calibrate_ransac_workspace_bytes(BATCH, POOL, ITER),
            "dcx_stereo_calibrate_pool": lambda: lib.dcx_stereo_calibrate_workspace_bytes(BATCH, POOL, POOL)}[entry]()


def _call(lib, entry, **bad):
    """The valid call of ``entry`` with the arguments named in ``bad`` replaced."""
    a = dict(counts=P, starts=P, rows=P, xy=P, counts1=P, starts1=P, rows1=P, batch=BATCH, pool=POOL, cols=5, rows_=4, square=0.01,
             camera=CAM, status=P, pose=P, info=P, result=RES, ws=P, ws_bytes=_ws_bytes(lib, entry) if ENTRIES[entry][1] else 0)
    a.update(bad)
    head = (a["counts"], a["starts"], a["rows"], a["xy"])
    board = (a["batch"], a["pool"], a["cols"], a["rows_"], a["square"])
    if entry == "dcx_solve_pnp_pool":
        return lib.dcx_solve_pnp_pool(*head, *board, a["camera"], None, 0, a["status"], a["pose"], None)
    if entry == "dcx_solve_pnp_ransac_pool":
        return lib.dcx_solve_pnp_ransac_pool(*head, *board, a["camera"], None, 0, ITER, 8.0, 4, 0, a["ws"], a["ws_bytes"], a["status"],
                                             a["pose"], a["info"], None, None)
    if entry == "dcx_calibrate_pool":
        return lib.dcx_calibrate_pool(*head, *board, 320, 240, a["ws"], a["ws_bytes"], a["status"], a["pose"], a["result"], None)
    if entry == "dcx_calibrate_ransac_pool":
        return lib.dcx_calibrate_ransac_pool(*head, *board, 320, 240, ITER, 8.0, 3.0, 6, 2, 0, a["ws"], a["ws_bytes"], a["status"],
                                             a["pose"], a["info"], None, a["result"], None)
    return lib.dcx_stereo_calibrate_pool(*head, None, a["counts1"], a["starts1"], a["rows1"], a["xy"], None, a["batch"], a["pool"],
                                         a["pool"], a["cols"], a["rows_"], a["square"], a["camera"], None, 0, a["camera"], None, 0,
                                         a["ws"], a["ws_bytes"], a["status"], a["pose"], a["info"], a["result"], None)


def _cases(lib, entry):
    """case name -> the arguments it makes bad"""
    own, has_ws, aligned = ENTRIES[entry]
    c = {f"null {p}": {p: None} for p in POOL_PTRS + own}
    c.update({"batch 0": dict(batch=0), "pool -1": dict(pool=-1), "col_count 1": dict(cols=1), "row_count 1": dict(rows_=1),
              "board over 2^31 - 1 ids": dict(cols=HUGE, rows_=HUGE), "square_len inf": dict(square=float("inf")),
              "square_len nan": dict(square=float("nan"))})
    if has_ws:
        c["workspace one byte short"] = dict(ws_bytes=_ws_bytes(lib, entry) - 1)
    if aligned:
        c["workspace misaligned by 4"] = dict(ws=P + 4)
    return c


def _short_ws(entry):
    return E_ARG if entry == "dcx_solve_pnp_ransac_pool" else E_WS


# recorded from the parent build: every refusal is DCX_E_ARG but the calibrations' short workspace
EXPECTED = {entry: {**{f"null {p}": E_ARG for p in POOL_PTRS + own},
                    **{k: E_ARG for k in ("batch 0", "pool -1", "col_count 1", "row_count 1", "board over 2^31 - 1 ids",
                                          "square_len inf", "square_len nan")},
                    **({"workspace one byte short": _short_ws(entry)} if has_ws else {}),
                    **({"workspace misaligned by 4": E_ARG} if aligned else {})}
            for entry, (own, has_ws, aligned) in ENTRIES.items()}


def test_pool_entries_refuse_bad_arguments_without_a_gpu():
    from deepcharuco_amd import _lib
    lib = _lib.lib()
    assert lib.dcx_error_string(E_ARG) != lib.dcx_error_string(E_WS)
    for entry in ENTRIES:
        if ENTRIES[entry][1]:
            assert 0 < _ws_bytes(lib, entry) <= len(_fake) - 8
        cases = _cases(lib, entry)
        assert set(cases) == set(EXPECTED[entry])
        got = {name: _call(lib, entry, **bad) for name, bad in cases.items()}
        print(entry, got)
        assert got == EXPECTED[entry], entry
    assert len(EXPECTED["dcx_stereo_calibrate_pool"]) == 20 and len(EXPECTED["dcx_solve_pnp_pool"]) == 13
