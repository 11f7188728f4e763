"""Times the fisheye pose solve and the fisheye calibration at 4,096 views beside their pinhole counterparts on the same scenes
(one MI355X) -> profiles/fisheye_probe.json.  No speed is promised anywhere; this is the measurement.

Scenes: 64 distinct noise-free views of an 8 x 5 board (28 corners) through a 230 px fisheye lens at 640 x 480, float32 pixels,
laid 64 times into one corner pool of 4,096 views.  The pinhole calls get the same pool: their camera cannot fit these pixels (that
is the point of the fisheye model), so their rows say what the same amount of data costs there, not that the answers agree.
Wall time around a synchronised call, median of ``--repeats`` after one warm-up call.

    python tools/fisheye_probe.py [--views 4096] [--repeats 7] [--out profiles/fisheye_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BOARD = (8, 5, 0.03)
SIZE = (640, 480)
K = np.array([[230.0, 0, 323.5], [0, 231.0, 236.5], [0, 0, 1]])
DIST = np.array([0.05, -0.01, 0.003, -0.0006])


def scenes(n, seed=1):
    from deepcharuco_amd import fisheye as fe, pnp
    rng = np.random.default_rng(seed)
    obj = pnp.object_points(np.arange(28), *BOARD).astype(np.float64)
    out = []
    while len(out) < n:
        r = rng.normal(size=3)
        r *= np.deg2rad(rng.uniform(3, 40)) / np.linalg.norm(r)
        z = rng.uniform(0.12, 0.3)
        t = np.array([rng.uniform(-0.35, 0.35) * z, rng.uniform(-0.35, 0.35) * z, z]) - pnp._rodrigues(r) @ np.array([0.075, 0.12, 0.0])
        pix = fe.project_points_host(obj, r, t, K, DIST)
        if np.isfinite(pix).all() and (pix >= 0).all() and (pix[:, 0] <= SIZE[0] - 1).all() and (pix[:, 1] <= SIZE[1] - 1).all():
            out.append(np.c_[pix.astype(np.float32).astype(np.float64), np.arange(28)])
    return out


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "fisheye_probe.json"))
    a = ap.parse_args()
    import torch
    from deepcharuco_amd import _lib, calib, corner_pool, fisheye as fe, pnp
    dev = torch.device("cuda", 0)
    base = scenes(64)
    frames = [base[i % 64] for i in range(a.views)]
    packed, b, pool = corner_pool.pack_keypoints(frames, dev)
    out_f = (torch.empty(b, dtype=torch.int32, device=dev), torch.empty((b, 8), dtype=torch.float64, device=dev))
    out_p = (torch.empty(b, dtype=torch.int32, device=dev), torch.empty((b, 8), dtype=torch.float64, device=dev))
    res = {"device": torch.cuda.get_device_name(0), "views": a.views, "rows_per_view": 28, "distinct_views": 64,
           "repeats": a.repeats, "csrc_sha256": _lib.csrc_sha256()}
    res["solve_pnp_fisheye_pool"] = timed(lambda: fe.solve_pnp_fisheye_pool(packed, b, pool, True, *BOARD, K, DIST, out=out_f), a.repeats)
    res["solve_pnp_pool (pinhole, no distortion)"] = timed(lambda: pnp.solve_pnp_pool(packed, b, pool, True, *BOARD, K, None, out=out_p),
                                                           a.repeats)
    res["fisheye frames solved"] = int((out_f[0] == 0).sum())
    res["pinhole frames solved"] = int((out_p[0] == 0).sum())
    cf = fe.calibrate_fisheye_pool(packed, b, pool, True, *BOARD, SIZE)
    cp = calib.calibrate_charuco_pool(packed, b, pool, True, *BOARD, SIZE)
    res["calibrate_fisheye_pool"] = dict(timed(lambda: fe.calibrate_fisheye_pool(packed, b, pool, True, *BOARD, SIZE), a.repeats),
                                         status=cf.status, steps=cf.iterations, attempts=cf.attempts, rms_px=cf.rms,
                                         fx=float(cf.camera_matrix[0, 0]))
    res["calibrate_charuco_pool (pinhole)"] = dict(timed(lambda: calib.calibrate_charuco_pool(packed, b, pool, True, *BOARD, SIZE),
                                                         a.repeats),
                                                   status=cp.status, steps=cp.iterations, attempts=cp.attempts, rms_px=cp.rms,
                                                   fx=float(cp.camera_matrix[0, 0]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
