"""Times the calibration with flags and with the rational model at 4,096 views beside the default call on the same pool (one
MI355X) -> profiles/calib_flags_probe.json.  No speed is promised anywhere; this is the measurement.

Scene: the wide-lens scene of tests/test_calib_flags_host.py (camera_exact.calib_views(7, n, K = 230 / 236 px at 640 x 480, all
eight distortion coefficients, the board at 0.10 - 0.16 m), 64 distinct noise-free views, float32 pixels, laid 64 times into one
corner pool of 4,096 views.  Variants:
  flags = 0                          dcx_calibrate_pool, the old entry (9 parameters; it cannot fit these pixels)
  FIX_K3 | ZERO_TANGENT_DIST         dcx_calibrate_flags_pool on the same per-view kernels, the masked reduce_solve
  USE_INTRINSIC_GUESS from the truth all eight coefficients given, so the 12-parameter kernels run with k4 k5 k6 held
  RATIONAL_MODEL                     the 12-parameter kernels from Zhang's start
Wall time around a synchronised call, median of ``--repeats`` after one warm-up call; steps, attempts and rms of each.  The one
comparison: ms per LM attempt of the flagged 9-parameter call against the default call in the same run (they run the same per-view
kernels; the calls differ in the number of attempts their data asks for).

    python tools/calib_flags_probe.py [--views 4096] [--repeats 7] [--out profiles/calib_flags_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZE = (640, 480)
K = np.array([[230.0, 0, 319.3], [0, 236.0, 238.1], [0, 0, 1]])
DIST = np.array([0.35, -0.08, 8e-4, -5e-4, 0.01, 0.7, 0.05, -0.01])


def timed(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calib_flags_probe.json"))
    a = ap.parse_args()
    import torch
    import camera_exact as cx
    from deepcharuco_amd import _lib, calib, corner_pool
    dev = torch.device("cuda", 0)
    _, imgs, ids_l, _ = cx.calib_views(7, 64, 0.0, K=K, dist=DIST, tz=(0.10, 0.16))
    base = [np.c_[m.astype(np.float64), i] for m, i in zip(imgs, ids_l)]
    frames = [base[i % 64] for i in range(a.views)]
    packed, b, pool = corner_pool.pack_keypoints(frames, dev)
    board = cx.CALIB_BOARD
    variants = {
        "flags = 0 (dcx_calibrate_pool)": {},
        "FIX_K3 | ZERO_TANGENT_DIST": dict(flags=calib.CALIB_FIX_K3 | calib.CALIB_ZERO_TANGENT_DIST),
        "USE_INTRINSIC_GUESS from the truth (8 coefficients, k4 k5 k6 held)": dict(flags=calib.CALIB_USE_INTRINSIC_GUESS, camera_matrix=K,
                                                                                  dist_coeffs=DIST),
        "RATIONAL_MODEL": dict(flags=calib.CALIB_RATIONAL_MODEL),
    }
    res = {"device": torch.cuda.get_device_name(0), "views": a.views, "distinct_views": 64, "rows": int(sum(len(f) for f in frames)),
           "repeats": a.repeats, "csrc_sha256": _lib.csrc_sha256()}
    for name, kw in variants.items():
        call = lambda: calib.calibrate_charuco_pool(packed, b, pool, True, *board, SIZE, **kw)      # noqa: E731
        r = call()
        t = timed(call, a.repeats)
        res[name] = dict(t, status=r.status, steps=r.iterations, attempts=r.attempts, rms_px=r.rms,
                         ms_per_attempt=round(t["median_ms"] / max(r.attempts, 1), 4), fx=float(r.camera_matrix[0, 0]),
                         dist=r.dist_coeffs.ravel().tolist())
    d, f = res["flags = 0 (dcx_calibrate_pool)"], res["FIX_K3 | ZERO_TANGENT_DIST"]
    res["ms per attempt, flagged 9-parameter call / default call"] = round(f["ms_per_attempt"] / d["ms_per_attempt"], 4)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
